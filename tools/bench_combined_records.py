#!/usr/bin/env python3
"""The `-a` flow to VCF lines: GT, GQ and GL per record formed on the device from the combined bins, against the route that
exists without it, on ONE resident job — tools/bench_combine.py's: C contigs x V variants x S subsets of 16 paths (a fifth of
the objects multiallelic), chain c * S + s = contig c over subset s, group c = its S chains.  Every contig has a record plan on
its first chain: a biallelic bubble is one record; a bubble of 3 .. 5 alleles is merged from two records (three for a quarter
of them) of two or three alleles each, one in fifty of the non-reference record alleles of undefined sequence.
One process, after a warm-up round, several repeats with their spread:

  (a) today's route: pg_job_fetch_combined_all (16 bytes x bins over PCIe), then per record on the host normalize ->
      fold onto the record's alleles -> get_specific_likelihoods -> likeliest genotype, quality, log10 and its four digits
      (pangenie_amd/genotyping_result.py in np.longdouble).  That loop is Python: it is timed on the first --host-variants
      bubbles of group 0 and the figure for the whole job is that time scaled by the number of records — an extrapolation,
      printed as one;
  (b) pg_job_combined_record_calls + pg_job_combined_record_gl + their two _all fetches (8 bytes a record, 4 a value).

Prints the two _ms values, pg_job_combined_calls_ms of the same job, and for the three lane-per-item kernels the bytes they
have to move by the traffic formulas below and the bytes/s that makes of their time:
    k_ccalls   variants x (16 + 8) + 16 x bins + 2 x alleles                                  (allele_off, geno_off; the bins; the ids; 8 out)
    k_crcalls  records x (44 + 8) + sum over records of (16 x bins(v) + 2 x A(v) + 2 x ids(r) + 2 x alleles(r))
    k_crgl     records x (44 + 16) + the same sum + 4 x values
(44: rec_var, two map_off, two vcf_off, two allele_off, two geno_off words; a bubble's bins count once per RECORD: every lane
reads its bubble's bins itself).  Checks on the first round that what (b) fetched is what (a) forms on its sample of bubbles.
Sets no threshold on time.

    python tools/bench_combined_records.py [--contigs 8] [--variants 100000] [--subsets 4] [--repeats 5] [--host-variants 20000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pangenie_amd import calls, hmm  # noqa: E402
from pangenie_amd.genotyping_result import GenotypingResult, fold_onto_record, record_call  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel  # noqa: E402
from tools.bench_combine import PATHS, spread, subset_batches  # noqa: E402

LD = np.longdouble


def make_plan(rng, batch):
    """the record plan described above"""
    aoff, aid = batch.allele_off.astype(np.int64), batch.allele_id
    bubbles = []
    for v in range(len(aoff) - 1):
        ids = aid[aoff[v]:aoff[v + 1]]
        n_ids = int(ids.max()) + 1
        if len(ids) <= 2:
            bubbles.append([(list(range(n_ids)) if n_ids <= 2 else [0] + [1] * (n_ids - 1), [True, True])])
            continue
        records = []
        for _ in range(3 if rng.random() < 0.25 else 2):
            nA = int(rng.integers(2, 4))
            own = rng.integers(0, nA, n_ids)
            own[0] = 0
            records.append((own.tolist(), [True] + [bool(x) for x in (rng.random(nA - 1) >= 0.02)]))
        bubbles.append(records)
    return calls.RecordPlan.from_records(bubbles)


def digits_text(x) -> str:
    with np.errstate(divide="ignore"):
        v = np.log10(LD(x))
    if np.isinf(v):
        return "-inf"
    if v == 0:
        return "0"
    return "%.4g" % float(np.format_float_scientific(v, precision=3, unique=False, trim="k"))


def host_records(batch, bins, plan, n_variants):
    """today's route for the first n_variants bubbles: per record (GT, GQ or None) and the texts of its GL values"""
    aoff, goff, ids = batch.allele_off.astype(np.int64), batch.geno_off.astype(np.int64), batch.allele_id
    val = calls.combined_to_longdouble(bins[:int(goff[n_variants])])
    present = bins["flags"][:int(goff[n_variants])] != 0
    out = []
    for v in range(n_variants):
        res = GenotypingResult()
        k = int(goff[v])
        A = int(aoff[v + 1] - aoff[v])
        for a in range(A):
            for b in range(a, A):
                if present[k]:
                    res.genotype_to_likelihood[(int(ids[aoff[v] + a]), int(ids[aoff[v] + b]))] = val[k]
                k += 1
        res.normalize()
        for r in range(int(plan.rec_off[v]), int(plan.rec_off[v + 1])):
            own, vcf = plan.record(r)
            g, gq = record_call(res, own, vcf)
            f = fold_onto_record(res, own)
            if f.contains_no_likelihoods():
                f.add_to_likelihood(0, 0, 1.0)
            defined = [a for a, x in enumerate(vcf) if int(x) != 0xFFFF]
            gl = f.get_specific_likelihoods(defined) if len(defined) < len(vcf) else f
            out.append((None if g is None else (int(g[0]), int(g[1]), int(gq)), [digits_text(x) for x in gl.get_all_likelihoods(len(defined))]))
    return out


def record_traffic(batch, plan):
    """the sum over the records of (16 x bins(v) + 2 x A(v) + 2 x ids(r) + 2 x alleles(r)), and the number of GL values"""
    A = np.diff(batch.allele_off.astype(np.int64))
    per = np.diff(plan.rec_off.astype(np.int64))
    Ar = np.repeat(A, per)
    return int((16 * (Ar * (Ar + 1) // 2) + 2 * Ar).sum() + 2 * int(plan.map_off[-1]) + 2 * int(plan.vcf_off[-1])), int(calls.record_gl_offsets(plan)[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--variants", type=int, default=100000)
    ap.add_argument("--subsets", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-variants", type=int, default=20000)
    args = ap.parse_args()
    C, V, S = args.contigs, args.variants, args.subsets
    fulls = [synthetic_panel(V, S * PATHS, 20, seed=19000 + c, multiallelic_frac=0.2) for c in range(C)]
    batches = [b for full in fulls for b in subset_batches(full, S)]
    groups = [[c * S + s for s in range(S)] for c in range(C)]
    rng = np.random.default_rng(20000)
    plans = [make_plan(rng, batches[g[0]]) for g in groups]
    n_records = sum(p.n_records for p in plans)
    multi = sum(int(np.diff(p.rec_off.astype(np.int64))[np.diff(p.rec_off.astype(np.int64)) > 1].sum()) for p in plans)
    job = hmm.Job(batches, hmm.ProbabilityTable(*default_table_args()), hmm.make_params(1.26, False, 1e-5))
    for g, plan in zip(groups, plans):
        job.record_plan(g[0], plan)
    job.run()
    job.combine_plan(groups)
    job.combine()
    n_bins = sum(int(batches[g[0]].geno_off[-1]) for g in groups)
    n_alleles = sum(int(batches[g[0]].allele_off[-1]) for g in groups)
    sums, values = zip(*[record_traffic(batches[g[0]], p) for g, p in zip(groups, plans)])
    n_values = sum(values)
    traffic = {"k_ccalls": C * V * 24 + 16 * n_bins + 2 * n_alleles, "k_crcalls": n_records * 52 + sum(sums),
               "k_crgl": n_records * 60 + sum(sums) + 4 * n_values}
    n_host = min(args.host_variants, V)
    host_share = int(plans[0].rec_off[n_host])
    t_dev, t_fetch, t_host, ms_calls, ms_gl, ms_ccalls = [], [], [], [], [], []
    for rep in range(args.repeats + 1):   # (the first round warms up: the buffers, the id check, the GQ table)
        t0 = time.perf_counter()
        recs = job.combined_record_calls()
        gls = job.combined_record_gl()
        t1 = time.perf_counter()
        bins = job.combined()
        t2 = time.perf_counter()
        want = host_records(batches[0], bins[0], plans[0], n_host)
        t3 = time.perf_counter()
        job.combined_calls()
        if rep == 0:
            gl_off = calls.record_gl_offsets(plans[0]).astype(np.int64)
            for r, (call, texts) in enumerate(want):
                got, fl = recs[0][r], int(recs[0][r]["flags"]) & 0xFF
                assert fl != calls.PG_CALL_DEFERRED
                assert (call is None) == (fl != calls.PG_CALL_OK) and (call is None or (int(got["allele_1"]), int(got["allele_2"]), int(got["gq"])) == call), (r, got, call)
                for x, t in zip(gls[0][gl_off[r]:gl_off[r + 1]], texts):
                    assert calls.gl_text(x) in (t, None), (r, x, t)
            continue
        t_dev.append(t1 - t0)
        t_fetch.append(t2 - t1)
        t_host.append(t3 - t2)
        ms_calls.append(job.combined_record_calls_ms() / 1e3)
        ms_gl.append(job.combined_record_gl_ms() / 1e3)
        ms_ccalls.append(job.combined_calls_ms() / 1e3)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    scale = n_records / host_share
    print(json.dumps({
        "shape": {"contigs": C, "variants": V, "subsets": S, "paths_per_subset": PATHS, "chains": C * S, "bins_per_subset": n_bins,
                  "records": n_records, "records_of_multi_record_bubbles": multi, "gl_values": n_values, "multiallelic_frac": 0.2},
        "pg_job_combined_record_calls_ms": spread(ms_calls), "pg_job_combined_record_gl_ms": spread(ms_gl),
        "pg_job_combined_calls_ms": spread(ms_ccalls),
        "formation_plus_both_fetch_all_wall": spread(t_dev),
        "today_fetch_combined_all_wall": spread(t_fetch),
        "today_host_formation_wall_of_the_sample": dict(spread(t_host), records=host_share),
        "today_host_formation_wall_extrapolated_to_all_records_ms": round(1e3 * med(t_host) * scale, 1),
        "traffic_bytes": traffic,
        "GB_per_s": {"k_ccalls": round(traffic["k_ccalls"] / med(ms_ccalls) / 1e9, 1), "k_crcalls": round(traffic["k_crcalls"] / med(ms_calls) / 1e9, 1),
                     "k_crgl": round(traffic["k_crgl"] / med(ms_gl) / 1e9, 1)},
        "ns_per_record": {"k_crcalls": round(1e9 * med(ms_calls) / n_records, 2), "k_crgl": round(1e9 * med(ms_gl) / n_records, 2),
                          "k_ccalls_per_variant": round(1e9 * med(ms_ccalls) / (C * V), 2)},
        "bytes_over_pcie": {"record_fields": 8 * n_records + 4 * n_values, "combined_bins": 16 * n_bins},
        "sample_checked_against_the_host_route": True,
    }, indent=1))
    job.close()


if __name__ == "__main__":
    main()
