"""Sampled cohorts end to end: pg_sampler_cohort_new (index once, counts per sample, costs on the device) against the route
available before it — pg_sampler_then_job over samples x contigs copies of the panel — on the same inputs, outputs asserted
identical.  Generator: tools/bench_sampler.py's (pangenie_amd.panel.synthetic_panel).
usage: python tools/bench_sampled_cohort.py [--samples 16,256] [--contigs 8] [--variants 8000] [--paths 215] [--size 15]
       [--check-chains 48] [--no-today] [--repeat 3]
Prints one JSON line per sample count.  (MEASUREMENT TOOL.)"""
import argparse, ctypes as C, json, sys, time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pangenie_amd import hmm  # noqa: E402
from pangenie_amd import sampler as smp  # noqa: E402
from pangenie_amd._lib import PgContigBatch  # noqa: E402
from pangenie_amd.panel import synthetic_panel  # noqa: E402

HBM_PEAK = 8.0e12   # MI355X, bytes/s


class _Panels:
    """job.batches on demand: a chain's reduced panel is read back only when a check fetches it"""
    def __init__(self, job):
        self.job, self.cache = job, {}

    def __getitem__(self, c):
        if c not in self.cache:
            self.cache[c] = self.job.fetch_panel(c)
        return self.cache[c]


def job_of(handle, table, params):
    j = hmm.Job.__new__(hmm.Job)
    j._lib, j.table, j.params, j.h, j._samples = smp._hip(), table, params, handle, None
    j.batches = _Panels(j)
    return j


def cohort_new(index, samples, size, table, params):
    lib = smp._hip()
    arr = (PgContigBatch * len(index))(*[b.as_c() for b in index])
    cs, keep = smp.marshal_samples(index, samples)
    err = C.create_string_buffer(1024)
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = lib.pg_sampler_cohort_new(0, len(index), arr, len(samples), cs, size, 1, 1.26, C.c_longdouble(25000.0), 10, table.h,
                                   C.byref(params), None, None, C.byref(h), err, 1024)
    wall = time.perf_counter() - t0
    if rc:
        raise hmm.PanGenieError(rc, err.value.decode(errors="replace"))
    del keep
    return job_of(h.value, table, params), wall


def then_job(index, samples, size, table, params):
    """today's route: every (sample, contig) as its own copy of the panel, one pg_sampler_then_job over all of them"""
    lib = smp._hip()
    copies = [b.with_counts(kc, cv) for (kcs, covs) in samples for b, kc, cv in zip(index, kcs, covs)]
    arr = (PgContigBatch * len(copies))(*[b.as_c() for b in copies])
    err = C.create_string_buffer(1024)
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = lib.pg_sampler_then_job(arr, len(copies), size, 1, 1.26, C.c_longdouble(25000.0), 10, table.h, C.byref(params), 0,
                                 None, None, C.byref(h), err, 1024)
    wall = time.perf_counter() - t0
    if rc:
        raise hmm.PanGenieError(rc, err.value.decode(errors="replace"))
    return job_of(h.value, table, params), wall


def draw(index, n, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([0, 1, 2, 3, 5, 9, 27], np.uint16)
    return [([rng.choice(vals, int(b.kmer_off[-1])) for b in index], [rng.integers(5, 40, b.n_variants).astype(np.uint16) for b in index])
            for _ in range(n)]


def forward_bytes(index, n_samples, size):
    """ks_forward_fast, from the shapes: per pass and chain it reads the cost words (V x T x 8 B) and the transition costs
    (V x 4 B) and writes the stay bits ((V - 1) / 16 x 2 x T x 4 B) and the minima (V x 4 B)"""
    total = 0
    for b in index:
        V, P = b.n_variants, b.n_paths
        NW = 1
        while NW * 256 < P:
            NW *= 2
        T = 64 * NW
        total += V * T * 8 + V * 4 + ((V + 14) // 16) * 2 * T * 4 + V * 4
    return total * n_samples * size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="16,256")
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--variants", type=int, default=8000)
    ap.add_argument("--paths", type=int, default=215)
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--check-chains", type=int, default=48)
    ap.add_argument("--no-today", action="store_true")
    ap.add_argument("--repeat", type=int, default=3, help="calls per route and sample count (the median is reported, every call listed)")
    a = ap.parse_args()
    index = [synthetic_panel(a.variants, a.paths, 20, seed=11 + g, multiallelic_frac=0.2) for g in range(a.contigs)]
    table = hmm.ProbabilityTable(4, 72, 36, 0.01)
    params = hmm.make_params(1.26, False, 1e-5)
    # warm-up (code objects, allocator) on both routes
    for fn in (cohort_new, then_job):
        j, _ = fn(index[:1], [(s[0][:1], s[1][:1]) for s in draw(index, 2, 1)], a.size, table, params)
        j.run()
        j.close()
    for ns in [int(x) for x in a.samples.split(",")]:
        samples = draw(index, ns, 100 + ns)
        V = a.variants * a.contigs * ns
        out = {"samples": ns, "contigs": a.contigs, "variants_per_contig": a.variants, "paths": a.paths, "size": a.size, "add_reference": True}
        walls, jn = [], []
        for _ in range(a.repeat - 1):   # (the call's time varies from call to call: repeated, the median run is the one kept)
            j, w = cohort_new(index, samples, a.size, table, params)
            walls.append(w)
            jn.append(smp.last_phase_ms()["job_new"])
            j.close()
        job, wall = cohort_new(index, samples, a.size, table, params)
        walls.append(wall)
        ph, (ms, kern), h2d = smp.last_phase_ms(), smp.last_ms(), smp.last_h2d_bytes()
        jn.append(ph["job_new"])
        out["cohort_new_calls_s"], out["cohort_new_job_new_ms"] = walls, jn
        out["cohort_new_job_alloc_s"] = job.host_seconds()["alloc_s"]
        wall = float(np.median(walls))
        t0 = time.perf_counter()
        job.run()
        run_s = time.perf_counter() - t0
        new = {"call_s": wall, "job_run_s": run_s, "variants_per_s_call": V / wall, "variants_per_s_end_to_end": V / (wall + run_s),
               "h2d_bytes_index": h2d[0], "h2d_bytes_per_sample_total": h2d[1], "h2d_bytes_per_sample": h2d[1] / ns,
               "phase_ms": ph, "pass_kernel_ms": {"expand": ms[0], "forward": ms[1], "backtrack_apply": ms[2]}, "fast_kernel_waves": kern,
               "job_index_ms": job.index_ms(), "job_kernel_ms": job.kernel_ms(), "job_device_bytes": job.device_bytes()}
        dev_ms = ph["cost_kernel"] + ph["slots"] + sum(ms) + job.index_ms()
        host_ms = ph["host_prep"] + max(0.0, ph["job_new"] - job.index_ms())
        new["host_ms_outside_device_waits_est"] = host_ms
        new["host_fraction_of_call_est"] = host_ms / ph["total"]
        new["device_ms_in_call"] = dev_ms
        fb = forward_bytes(index, ns, a.size)
        new["forward_bytes"] = fb
        new["forward_hbm_fraction"] = fb / (ms[1] * 1e-3) / HBM_PEAK if ms[1] > 0 else None
        out["cohort_new"] = new
        if not a.no_today:
            owalls = []
            for _ in range(a.repeat - 1):
                j, w = then_job(index, samples, a.size, table, params)
                owalls.append(w)
                j.close()
            old_job, old_wall = then_job(index, samples, a.size, table, params)
            owalls.append(old_wall)
            out["then_job_calls_s"] = owalls
            old_wall = float(np.median(owalls))
            (oms, _), oh2d = smp.last_ms(), smp.last_h2d_bytes()
            t0 = time.perf_counter()
            old_job.run()
            old_run = time.perf_counter() - t0
            out["then_job_copies"] = {"call_s": old_wall, "job_run_s": old_run, "variants_per_s_call": V / old_wall,
                                      "variants_per_s_end_to_end": V / (old_wall + old_run), "h2d_bytes_index": oh2d[0],
                                      "h2d_bytes_per_sample_total": oh2d[1],
                                      "pass_kernel_ms": {"expand": oms[0], "forward": oms[1], "backtrack_apply": oms[2]}}
            out["speedup_call"] = old_wall / wall
            out["speedup_end_to_end"] = (old_wall + old_run) / (wall + run_s)
            # outputs identical: reduced panels and posteriors of a spread of chains
            n = ns * a.contigs
            chains = sorted(set(np.linspace(0, n - 1, min(a.check_chains, n)).astype(int).tolist()))
            for c in chains:
                p, q = job.batches[c], old_job.batches[c]
                for f in ("kmer_off", "kmer_count", "allele_off", "allele_id", "allele_flags", "allele_kmer_off", "allele_kmer_mask", "path_allele"):
                    assert np.array_equal(getattr(p, f), getattr(q, f)), (c, f)
                r, w = job.fetch(c), old_job.fetch(c)
                assert r.n_columns == w.n_columns and np.array_equal(r.lik, w.lik) and np.array_equal(r.lik_exp, w.lik_exp), c
                assert np.array_equal(r.kept, w.kept) and np.array_equal(r.coverage, w.coverage) and np.array_equal(r.n_kmers, w.n_kmers), c
            out["checked_chains_identical"] = len(chains)
            old_job.close()
        job.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
