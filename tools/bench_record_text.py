#!/usr/bin/env python3
"""The bytes of the sample column `GT:GQ:GL:KC` of a SAMPLED cohort: two routes from one job that has run to
the text of every record of every chain, on the `small` shape of tools/bench_sampled_record_fields.py (64 samples x 8 contigs x
2 000 bubbles, 128 paths sampled to 15 + 1, its plan).  One process, one warm-up, several repeats with their spread.

  (b)  as it stands: pg_job_record_calls + pg_job_record_gl, the two packed fetches, then the C++ host forms every sample
       column — pangenie::record_field_text, the ostringstream and one pg_gl_text per value that Graph::genotypes_records runs
       per record — on 1 and on 16 threads (tools/record_text_host_bench.cpp, a program of its own: it reads the fetched
       fields from a file, so its time is the formation alone);
  (c)  pg_job_record_text (which forms calls and values where they are not formed for this run: here they are, so its time
       is the text's own) + the packed fetch of the bytes and their offsets.

Asserts that both routes give the same bytes.  Prints one JSON line: median [min .. max] of each part, the bytes over PCIe per
record, and k_rtext_emit's achieved GB/s against its formula traffic (what it reads per record and value + the text and the
offsets it writes).  Sets no threshold on time.

    python tools/bench_record_text.py --shape tiny|small [--repeats N] [--build-only]
"""
import argparse
import ctypes as C
import json
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_record_calls import random_plan  # noqa: E402
from bench_sampled_record_fields import PATHS, SHAPES, SIZE, form  # noqa: E402
from pangenie_amd import build, calls, hmm  # noqa: E402
from pangenie_amd import sampler as smp  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402

HOST_BENCH = ROOT / "tools" / "_build" / "record_text_host_bench.bin"


def build_host_bench() -> Path:
    build.build_host()
    src = ROOT / "tools" / "record_text_host_bench.cpp"
    if not HOST_BENCH.exists() or HOST_BENCH.stat().st_mtime < max(src.stat().st_mtime, build.HOST_LIB.stat().st_mtime):
        HOST_BENCH.parent.mkdir(parents=True, exist_ok=True)
        host, csrc = ROOT / "pangenie_amd" / "host", ROOT / "pangenie_amd" / "csrc"
        cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", str(src), "-o", str(HOST_BENCH), f"-L{host}", "-lpangenie_host", f"-L{csrc}",
               "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", "-Wl,-rpath,$ORIGIN/../../pangenie_amd/host:$ORIGIN/../../pangenie_amd/csrc"]
        subprocess.run(cmd, check=True)
    return HOST_BENCH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["tiny", "small"], default="small")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--build-only", action="store_true", help="build tools/_build/record_text_host_bench.bin and leave")
    args = ap.parse_args()
    exe = build_host_bench()
    if args.build_only:
        return
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
    plans = [random_plan(rng, ix) for ix in index]
    offsets = [calls.record_gl_offsets(p) for p in plans]
    rec_var = [np.repeat(np.arange(p.n_variants), np.diff(p.rec_off.astype(np.int64))) for p in plans]
    for _ in range(2):
        job.run()
    for i in range(nc):
        job.record_plan_strided(i, nc, plans[i])
    lib, err = job._lib, C.create_string_buffer(1024)

    def text():
        if lib.pg_job_record_text(job.h, 0, err, 1024):
            raise RuntimeError(err.value.decode(errors="replace"))

    T = {k: [] for k in ("b_form", "b_fetch", "c_form", "c_fetch")}
    ms = {k: [] for k in ("record_calls", "record_gl", "record_text", "rtext_emit")}
    b = got = None
    for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
        t0 = time.perf_counter()
        form(job)
        t1 = time.perf_counter()
        b = (job.record_calls_packed(), job.record_gl_packed())
        t2 = time.perf_counter()
        text()
        t3 = time.perf_counter()
        got = calls.fetch_record_text_packed(job)
        t4 = time.perf_counter()
        if rep:
            for k, v in zip(("b_form", "b_fetch", "c_form", "c_fetch"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                T[k].append(v)
            ms["record_calls"].append(job.record_calls_ms()); ms["record_gl"].append(job.record_gl_ms())
            ms["record_text"].append(job.record_text_ms()); ms["rtext_emit"].append(float(lib.pg_job_record_text_emit_ms(job.h)))
    (packed, first), (packed_gl, first_gl) = b
    off, text_bytes, text_first = got
    n_rec, n_val = len(packed), len(packed_gl)
    # route (b)'s host part: the fetched fields and, per record, KC and UK == 0 (pg_job_fetch's, host memory) to a file
    with tempfile.TemporaryDirectory() as tmp:
        fields, out = Path(tmp) / "fields.bin", Path(tmp) / "text.bin"
        with open(fields, "wb") as f:
            np.array([n], np.uint64).tofile(f)
            for g in range(n):
                rc, gl = packed[int(first[g]):int(first[g + 1])], packed_gl[int(first_gl[g]):int(first_gl[g + 1])]
                res = job.fetch(g)
                np.array([len(rc), len(gl)], np.uint64).tofile(f)
                rc.tofile(f); offsets[g % nc].astype(np.uint64).tofile(f); gl.tofile(f)
                res.coverage[rec_var[g % nc]].astype(np.uint16).tofile(f)
                np.zeros(len(rc), np.uint8).tofile(f)   # (ignore_imputed off: no record is a no-call for its k-mers)
        r = subprocess.run([str(exe), str(fields), str(out), str(args.repeats), "1", "16"], capture_output=True, text=True, check=True)
        host = json.loads(r.stdout.strip().splitlines()[-1])
        host_text = out.read_bytes()
    assert host_text == text_bytes, (len(host_text), len(text_bytes))   # both routes: the same bytes
    assert int(off[-1]) == len(text_bytes) == int(text_first[-1]) and len(off) == n_rec + 1
    empty = int((np.diff(off.astype(np.int64)) == 0).sum())
    job.close()
    sp = lambda xs: {"median_ms": round(1e3 * float(np.median(xs)), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}
    kms = lambda xs: {"median": round(float(np.median(xs)), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}
    # k_rtext_emit per record: the call 8, two offsets of its values 8 (shared with the neighbour), the bubble 4, KC 2, the bubble's
    # k-mer offsets 8, its place in the block 4; per value 4; written: the text and one 64-bit offset per record
    traffic = (8 + 8 + 4 + 2 + 8 + 4) * n_rec + 4 * n_val + len(text_bytes) + 8 * n_rec
    emit = float(np.median(ms["rtext_emit"]))
    res = {"shape": args.shape, "chains": n, "records": n_rec, "gl_values": n_val, "text_bytes": len(text_bytes), "records_left_to_the_host": empty,
           "repeats": args.repeats, "routes_agree": True}
    res.update({k: sp(v) for k, v in T.items()})
    res.update({"b_host_1_thread": host["threads_1"], "b_host_16_threads": host["threads_16"],
                "pg_job_record_calls_ms": kms(ms["record_calls"]), "pg_job_record_gl_ms": kms(ms["record_gl"]), "pg_job_record_text_ms": kms(ms["record_text"]),
                "k_rtext_emit_ms": kms(ms["rtext_emit"]), "k_rtext_emit_formula_bytes": traffic, "k_rtext_emit_GBps": round(traffic / emit / 1e6, 1) if emit > 0 else None,
                "bytes_per_record_b": round((8.0 * n_rec + 4.0 * n_val) / n_rec, 2), "bytes_per_record_c": round((len(text_bytes) + 8.0 * (n_rec + 1)) / n_rec, 2)})
    b_total = float(np.median(T["b_form"])) + float(np.median(T["b_fetch"]))
    c_extra = float(np.median(T["c_form"])) + float(np.median(T["c_fetch"]))
    res["route_b_ms"] = {"device_and_fetch": round(1e3 * b_total, 3), "with_host_1_thread": round(1e3 * b_total + host["threads_1"]["median_ms"], 3),
                         "with_host_16_threads": round(1e3 * b_total + host["threads_16"]["median_ms"], 3)}
    res["route_c_ms"] = {"both_formations": round(1e3 * float(np.median(T["b_form"])), 3), "text_and_fetch": round(1e3 * c_extra, 3),
                         "total": round(1e3 * (float(np.median(T["b_form"])) + c_extra), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
