#!/usr/bin/env python
"""A sample's kmer_count / coverage arrays: the host loop against the count plan, one JSON line per item.

Input is made on the spot by tools/simulate_pangenome.py and indexed by tests/cpp/test_host.bin (shapes of
tools/bench_kmer_counter.py); tools/count_fill_bench.cpp measures in ONE process after ONE count():
  add_targets_from_table_alone / plan_construction   once per index
  plan_fill / plan_fill_job                          per sample: wall seconds, kernel ms (events), bytes crossing PCIe
  host_route                                         first getKmerAbundance (table fetch) + fill_read_kmercounts_all at 16
                                                     threads + SampleCounts::of, and whether plan_fill gave the same arrays
usage: tools/bench_count_fill.py [--shape full|small] [--out FILE] [--keep DIR] [--build-only] [--prepare-only]
"""
import argparse
import json
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SHAPES = {"full": (20000000, 40000, 32, 30), "small": (2000000, 4000, 32, 30)}


def driver() -> Path:
    from pangenie_amd import build
    build.build_host()
    exe, src = ROOT / "tools" / "count_fill_bench.bin", ROOT / "tools" / "count_fill_bench.cpp"
    if build._stale(exe, [src, build.HOST_LIB]):
        host, csrc = build.HOST_DIR, build.CSRC
        cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", str(src), "-o", str(exe), f"-L{host}", "-lpangenie_host",
               f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-Wl,-rpath,$ORIGIN/../pangenie_amd/host:$ORIGIN/../pangenie_amd/csrc"]
        subprocess.run(cmd, check=True)
    return exe


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="full")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--keep", default=None, help="work directory to keep (default: a temporary one, removed)")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--prepare-only", action="store_true", help="make the inputs in --keep DIR and stop")
    a = ap.parse_args()
    exe = driver()
    if a.build_only:
        print(exe)
        return 0
    length, records, samples, coverage = SHAPES[a.shape]
    work = Path(a.keep) if a.keep else Path(tempfile.mkdtemp(prefix="pg_count_fill."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        if not (work / "idx_UniqueKmersMap.cereal").exists():
            sim = [sys.executable, str(ROOT / "tools" / "simulate_pangenome.py")]
            subprocess.run(sim + ["panel", str(length), str(records), str(samples), "11", str(work / "q")], check=True, stdout=subprocess.DEVNULL)
            subprocess.run(sim + ["sample", str(work / "q"), str(coverage), "5"], check=True, stdout=subprocess.DEVNULL)
            subprocess.run([str(ROOT / "tests" / "cpp" / "test_host.bin"), "index", str(work / "q.fa"), str(work / "q.vcf"), str(work / "idx"), "31", "0"],
                           check=True, stdout=subprocess.DEVNULL)
        if a.prepare_only:
            return 0
        head = {"what": "input", "shape": a.shape, "genome_bases": length, "records": records, "panel_samples": samples, "coverage": coverage,
                "reads_bytes": (work / "q_reads.fa").stat().st_size, "k": 31}
        lines = [json.dumps(head)]
        print(lines[0], flush=True)
        p = subprocess.Popen([str(exe), str(work / "idx"), str(work / "q_reads.fa"), str(coverage)], stdout=subprocess.PIPE, text=True)
        for line in p.stdout:
            line = line.strip()
            if line.startswith("{"):
                json.loads(line)
                lines.append(line)
            print(line, flush=True)
        rc = p.wait()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return rc
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
