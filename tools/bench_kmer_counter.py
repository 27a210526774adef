#!/usr/bin/env python
"""Where a sample's read counting stands, host against device: one JSON line per measurement.

Input is made on the spot by tools/simulate_pangenome.py (nothing downloaded) and indexed by tests/cpp/test_host.bin; the
measurements are taken by tools/kmer_counter_bench.cpp in ONE process:
  reader_alone              records parsed and batched, batches dropped: the ceiling of any design with one host reader
  host_targeted_count       TargetedKmerCounter::count at 16 threads and at 1
  device_count_end_to_end   DeviceKmerCounter::count, pageable file to synced counts; later rounds: the next samples (reset_counts)
  count_kernel_resident     kk_count alone on text resident in HBM, for the graph's segments (most windows hit) and for the
                            table's k-mers only (most miss)
usage: tools/bench_kmer_counter.py [--shape full|small] [--out FILE] [--keep DIR] [--prepare-only]
  full  = the 20 Mb / 30x shape of tools/pipeline_check.sh (589 MB of reads); small = 2 Mb / 30x
The kernel table comes from `tools/profile.sh kmers <tag>` (rocprofv3 --kernel-trace --stats around the C++ driver, device lines only).
"""
import argparse
import glob
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
    exe, src = ROOT / "tools" / "kmer_counter_bench.bin", ROOT / "tools" / "kmer_counter_bench.cpp"
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
    ap.add_argument("--prepare-only", action="store_true", help="make the inputs in --keep DIR and stop (tools/profile.sh kmers)")
    a = ap.parse_args()
    exe = driver()
    if a.build_only:
        print(exe)
        return 0
    length, records, samples, coverage = SHAPES[a.shape]
    work = Path(a.keep) if a.keep else Path(tempfile.mkdtemp(prefix="pg_kmer_bench."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        sim = [sys.executable, str(ROOT / "tools" / "simulate_pangenome.py")]
        subprocess.run(sim + ["panel", str(length), str(records), str(samples), "11", str(work / "q")], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(sim + ["sample", str(work / "q"), str(coverage), "5"], check=True, stdout=subprocess.DEVNULL)
        subprocess.run([str(ROOT / "tests" / "cpp" / "test_host.bin"), "index", str(work / "q.fa"), str(work / "q.vcf"), str(work / "idx"), "31", "0"],
                       check=True, stdout=subprocess.DEVNULL)
        tables = sorted(glob.glob(str(work / "idx_*_kmers.tsv.gz")))
        if a.prepare_only:
            return 0
        head = {"what": "input", "shape": a.shape, "genome_bases": length, "records": records, "panel_samples": samples, "coverage": coverage,
                "reads_bytes": (work / "q_reads.fa").stat().st_size, "k": 31}
        lines = [json.dumps(head)]
        print(lines[0], flush=True)
        p = subprocess.Popen([str(exe), "31", str(work / "idx_path_segments.fasta"), str(work / "q_reads.fa"), *tables], stdout=subprocess.PIPE, text=True)
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
