#!/usr/bin/env python
"""A sampled cohort batch from counted reads: the two routes from the counter's table to a sampled job, one
JSON line per item.

Input is made on the spot by tools/simulate_pangenome.py and indexed by tests/cpp/test_host.bin (shapes of
tools/bench_count_fill.py).  ONE process, ONE count() of the reads; a handful of samples are formed from that table at
different k-mer coverages.  Per repeat and route, for the whole batch:
  (a) host    CountPlan.fill (pg_count_plan_fill_host) per sample -> host arrays -> sample_cohort (pg_sampler_cohort_new)
  (b) device  CountPlan.fill_device(out = a SamplerCounts row) per sample -> sample_cohort_device (pg_sampler_cohort_new_device)
Reported per sample: wall seconds (median, min, max over the repeats after a warm-up), the bytes that cross PCIe for the
per-sample arrays, and the eight pg_sampler_last_phase_ms slots of the last repeat.  What can be derived is asserted: route
(b) uploads 0 bytes of per-sample arrays, and both routes' jobs answer the same results.  The time saved has no threshold:
route (a) in the same run is the yardstick.
usage: tools/bench_sampled_reads.py [--shape small|full] [--samples N] [--size N] [--repeats N] [--out FILE] [--keep DIR]
"""
import argparse
import json
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SHAPES = {"full": (20000000, 40000, 64, 30), "small": (2000000, 4000, 32, 30)}


def sequences(path: Path) -> bytes:
    """the sequence lines of a FASTA file, a newline after each"""
    return b"".join(line for line in path.open("rb") if not line.startswith(b">"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="full")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--size", type=int, default=15, help="sampled paths per variant (the reference path is added)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--keep", default=None, help="work directory to keep (default: a temporary one, removed)")
    a = ap.parse_args()
    import numpy as np
    from pangenie_amd import build, cereal_io, hmm, kmers
    from pangenie_amd import panel as pn
    from pangenie_amd import sampler as smp
    build.build_host()
    length, records, panel_samples, coverage = SHAPES[a.shape]
    work = Path(a.keep) if a.keep else Path(tempfile.mkdtemp(prefix="pg_sampled_reads."))
    work.mkdir(parents=True, exist_ok=True)
    lines = []

    def say(**item):
        lines.append(json.dumps(item))
        print(lines[-1], flush=True)

    try:
        if not (work / "idx_UniqueKmersMap.cereal").exists():
            sim = [sys.executable, str(ROOT / "tools" / "simulate_pangenome.py")]
            subprocess.run(sim + ["panel", str(length), str(records), str(panel_samples), "11", str(work / "q")], check=True, stdout=subprocess.DEVNULL)
            subprocess.run(sim + ["sample", str(work / "q"), str(coverage), "5"], check=True, stdout=subprocess.DEVNULL)
            subprocess.run([str(build.HOST_TEST), "index", str(work / "q.fa"), str(work / "q.vcf"), str(work / "idx"), "31", "0"],
                           check=True, stdout=subprocess.DEVNULL)
        m = cereal_io.load(work / "idx_UniqueKmersMap.cereal")
        names = sorted(m.unique_kmers)
        index = [pn.flatten(m.unique_kmers[c]) for c in names]
        tables = [work / f"idx_{c}_kmers.tsv.gz" for c in names]
        sumK, V = sum(int(b.kmer_off[-1]) for b in index), sum(b.n_variants for b in index)
        say(what="input", shape=a.shape, genome_bases=length, records=records, paths=int(index[0].n_paths), contigs=len(index), variants=V,
            unique_kmers=sumK, coverage=coverage, reads_bytes=(work / "q_reads.fa").stat().st_size, k=31, samples=a.samples, size=a.size,
            repeats=a.repeats)
        contigs = [kmers.parse_kmer_table(t, 31) for t in tables]
        text = sequences(work / "q_reads.fa")
        table = hmm.ProbabilityTable(coverage // 4, coverage * 4, 2 * coverage, 0.01)
        params = hmm.make_params(1.26, False, 1e-5)
        S = a.samples
        coverages = [coverage - s for s in range(S)]
        with kmers.KmerCounter(31) as counter:
            for c in contigs:
                for codes in (c.kmer_code, c.flank_code):
                    counter.add_codes(codes[codes != np.uint64(kmers.NOT_REGISTERED)])
            t0 = time.perf_counter()
            counter.count(text)
            say(what="count", seconds=time.perf_counter() - t0, text_bytes=len(text))
            with kmers.CountPlan(counter, contigs) as plan, smp.SamplerCounts(index, S) as counts:
                def route_host():
                    t0 = time.perf_counter()
                    filled = [plan.fill(cv) for cv in coverages]
                    t1 = time.perf_counter()
                    made = smp.sample_cohort(index, filled, a.size, table, params, add_reference=True, want_paths=False)
                    return made[0], t1 - t0, time.perf_counter() - t1, smp.last_h2d_bytes(), smp.last_phase_ms()

                def route_device():
                    t0 = time.perf_counter()
                    for s, cv in enumerate(coverages):
                        plan.fill_device(cv, out=counts.rows(s))
                    t1 = time.perf_counter()
                    made = smp.sample_cohort_device(index, counts, a.size, table, params, add_reference=True, want_paths=False)
                    return made[0], t1 - t0, time.perf_counter() - t1, smp.last_h2d_bytes(), smp.last_phase_ms()

                results = {}
                for name, route in (("host", route_host), ("device", route_device)):
                    fills, builds, runs = [], [], []
                    for rep in range(a.repeats + 1):   # (the first one warms up and is dropped)
                        job, t_fill, t_build, h2d, phases = route()
                        t0 = time.perf_counter()
                        job.run()
                        got = job.fetch_all()
                        t_run = time.perf_counter() - t0
                        if rep == a.repeats:
                            results[name] = [(r.n_columns, r.lik.copy(), r.lik_exp.copy(), r.coverage.copy()) for r in got]
                        job.close()
                        if rep:
                            fills.append(t_fill / S); builds.append(t_build / S); runs.append(t_run / S)
                    total = [f + b for f, b in zip(fills, builds)]
                    stat = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
                    # per sample: what the fill brings back and the cohort call sends up again (a), or nothing but the coverage (b)
                    d2h = 2 * sumK + 2 * V if name == "host" else 2 * V
                    h2d_sample = h2d[1] // S + (2 * V if name == "host" else 2 * V)   # (+ the coverage pg_job_new uploads, both routes)
                    if name == "device":
                        assert h2d[1] == 0, h2d
                    else:
                        assert h2d[1] == S * 2 * sumK, h2d
                    say(what="route", route=name, seconds_per_sample=stat(total), fill_seconds_per_sample=stat(fills),
                        cohort_new_seconds_per_sample=stat(builds), run_fetch_seconds_per_sample=stat(runs), index_h2d_bytes=h2d[0],
                        per_sample_h2d_bytes=h2d_sample, per_sample_array_upload_bytes=h2d[1] // S, per_sample_d2h_bytes=d2h, phase_ms=phases)
                same = all(a_[0] == b_[0] and all(np.array_equal(x, y) for x, y in zip(a_[1:], b_[1:])) for a_, b_ in zip(results["host"], results["device"]))
                assert same and len(results["host"]) == len(results["device"]), "the two routes' jobs answered different results"
                say(what="check", same_results=same, chains=len(results["host"]))
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return 0
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
