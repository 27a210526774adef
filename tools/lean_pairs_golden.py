#!/usr/bin/env python3
"""Writes tests/golden/lean_pairs_parent.npz: lik, lik_exp and kept of the six small chains of tests/test_lean_pairs_gpu.py
(golden_chains: their seeds and column counts stand there), each run as a job of its own at PG_SWEEP_MODE=chunked, PG_CHUNK_COLS=64,
PG_PIECE_CHUNKS=1 — pieces of phase 1, chunk sweeps, refill segments and the launches without a step all occur.

Run on the device with the native library of the commit whose results are to be pinned — a checkout of it, or PANGENIE_HMM_LIB
naming a libpangenie_hmm.so built from it; the committed file was written with the library of the commit before the lean-pairs
change (e5bf9ec).  The chains are built on the host from their seeds and do not depend on the library.

    python tools/lean_pairs_golden.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from oracle import pyoracle  # noqa: E402
from tests.test_lean_pairs_gpu import GOLDEN, golden_chains, run_golden  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else str(GOLDEN)
    chains = golden_chains(pyoracle)
    got = run_golden(chains, 64, 1, os.environ.__setitem__)
    again = run_golden(chains, 128, 2, os.environ.__setitem__)
    arrays = {"names": np.array(sorted(got))}
    for name, r in got.items():
        assert r.lik.tobytes() == again[name].lik.tobytes() and np.array_equal(r.lik_exp, again[name].lik_exp), name
        arrays[name + ".lik"] = np.asarray(r.lik, dtype=np.float64)
        arrays[name + ".lik_exp"] = np.asarray(r.lik_exp)
        arrays[name + ".kept"] = np.asarray(r.kept)
        print(f"{name}: {r.n_columns} columns, {r.lik.size} bins")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
