#!/usr/bin/env python3
"""Path subsets combined on the device against the route that exists without it, on ONE resident job: C contigs x V variants x
S subsets of 16 paths (a fifth of the objects multiallelic), chain c * S + s = contig c over subset s, group c = its S chains.
One process, after a warm-up, several repeats with their spread:

  (a) the route of a caller who adds up on the host: pg_job_fetch_all of the member chains (12 bytes x bins x subsets over
      PCIe), then GenotypingResult::combine per key in long double (vectorised numpy over all bins of a group at once: the same
      additions in the same order; what the index alone decides — which slots a bin belongs to — is prepared outside the timing);
  (b) pg_job_combine + pg_job_fetch_combined_all (16 bytes x bins).

Prints pg_job_combine_ms and pg_job_combined_calls_ms, the bytes k_combine has to move by the traffic formula
    bins x (12 S + 16) + S x (variants + alleles)          (the bins of S chains in, one combined bin out, the presence bytes)
and the bytes/s that makes of pg_job_combine_ms, and asserts that the two routes give the same bits for every bin.
Sets no threshold on time.

    python tools/bench_combine.py [--contigs 8] [--variants 100000] [--subsets 4] [--repeats 5]
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
from pangenie_amd.panel import ContigBatch, default_table_args, synthetic_panel  # noqa: E402

LD = np.longdouble
PATHS = 16


def subset_batches(full, S):
    """what panel.flatten(objects, only_paths) gives for S runs of 16 paths: the index arrays hang on the objects, the paths are chosen"""
    V = full.n_variants
    pa = full.path_allele.reshape(V, full.n_paths)
    return [ContigBatch(PATHS, full.variant_pos, full.coverage, full.kmer_off, full.kmer_count, full.allele_off, full.allele_id, full.allele_flags,
                        full.allele_kmer_off, full.allele_kmer_mask, np.ascontiguousarray(pa[:, s * PATHS:(s + 1) * PATHS]).reshape(-1)) for s in range(S)]


def bin_slots(batch):
    """per bin: its variant and the two allele slots (global indices into allele_present) it belongs to"""
    aoff = batch.allele_off.astype(np.int64)
    A = np.diff(aoff)
    var, sa, sb = [], [], []
    for a in np.unique(A):
        vs = np.flatnonzero(A == a)
        x, y = np.triu_indices(int(a))
        var.append(np.repeat(vs, len(x)))
        sa.append((aoff[vs][:, None] + x[None, :]).reshape(-1))
        sb.append((aoff[vs][:, None] + y[None, :]).reshape(-1))
    var, sa, sb = np.concatenate(var), np.concatenate(sa), np.concatenate(sb)
    goff = batch.geno_off.astype(np.int64)
    # bins in the job's order: variant after variant, row after row
    order = np.lexsort((sb, sa, var))
    assert len(order) == int(goff[-1])
    return var[order], sa[order], sb[order]


def host_combine(results, slots):
    """GenotypingResult::combine over the chains of one group, in their order: (present, value)"""
    var, sa, sb = slots
    total = np.zeros(len(var), LD)
    present = np.zeros(len(var), bool)
    for r in results:
        held = r.kept[var].astype(bool) & r.allele_present[sa].astype(bool) & r.allele_present[sb].astype(bool)
        value = np.ldexp(r.lik.astype(LD), r.lik_exp.astype(np.int64))
        total = np.where(held, total + value, total)
        present |= held
    return present, total


def spread(xs):
    xs = sorted(xs)
    return {"median_ms": round(1e3 * xs[len(xs) // 2], 3), "min_ms": round(1e3 * xs[0], 3), "max_ms": round(1e3 * xs[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--variants", type=int, default=100000)
    ap.add_argument("--subsets", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    C, V, S = args.contigs, args.variants, args.subsets
    fulls = [synthetic_panel(V, S * PATHS, 20, seed=19000 + c, multiallelic_frac=0.2) for c in range(C)]
    batches = [b for full in fulls for b in subset_batches(full, S)]
    groups = [[c * S + s for s in range(S)] for c in range(C)]
    slots = [bin_slots(batches[g[0]]) for g in groups]
    job = hmm.Job(batches, hmm.ProbabilityTable(*default_table_args()), hmm.make_params(1.26, False, 1e-5))
    job.run()
    job.combine_plan(groups)
    n_bins = sum(int(batches[g[0]].geno_off[-1]) for g in groups)
    n_alleles = sum(int(batches[g[0]].allele_off[-1]) for g in groups)
    traffic = n_bins * (12 * S + 16) + S * (C * V + n_alleles)
    into = [hmm.ContigResult(b) for b in batches]
    t_host_fetch, t_host_add, t_dev, ms_combine, ms_calls = [], [], [], [], []
    for rep in range(args.repeats + 1):   # (the first round warms up: buffers, pinned staging, the GQ table)
        t0 = time.perf_counter()
        res = job.fetch_all(into)
        t1 = time.perf_counter()
        want = [host_combine([res[c] for c in g], sl) for g, sl in zip(groups, slots)]
        t2 = time.perf_counter()
        job.combine()
        got = job.combined()
        t3 = time.perf_counter()
        job.combined_calls()
        if rep == 0:
            for (present, total), bins in zip(want, got):
                deferred = (bins["flags"] & calls.PG_COMBINED_DEFERRED) != 0
                assert not deferred.any()
                assert np.array_equal(present, bins["flags"] != 0)
                assert (calls.combined_to_longdouble(bins)[present] == total[present]).all()
            continue
        t_host_fetch.append(t1 - t0)
        t_host_add.append(t2 - t1)
        t_dev.append(t3 - t2)
        ms_combine.append(job.combine_ms() / 1e3)
        ms_calls.append(job.combined_calls_ms() / 1e3)
    med = sorted(ms_combine)[len(ms_combine) // 2]
    print(json.dumps({
        "shape": {"contigs": C, "variants": V, "subsets": S, "paths_per_subset": PATHS, "chains": C * S, "bins_per_subset": n_bins,
                  "multiallelic_frac": 0.2},
        "pg_job_combine_ms": spread(ms_combine), "pg_job_combined_calls_ms": spread(ms_calls),
        "combine_plus_fetch_combined_all_wall": spread(t_dev),
        "host_route_fetch_all_wall": spread(t_host_fetch), "host_route_additions_wall": spread(t_host_add),
        "k_combine_traffic_bytes": traffic, "k_combine_GB_per_s": round(traffic / med / 1e9, 1),
        "bytes_over_pcie": {"combined": 16 * n_bins, "host_route": 12 * S * n_bins},
        "identical_bits": True,
    }, indent=1))
    job.close()


if __name__ == "__main__":
    main()
