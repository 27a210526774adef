"""bench.py as a plain run (the main workload's steps and nothing else) and its --dump-outputs, on a small workload: one
JSON line with the headline fields and none of the --full measurements, and the same outputs from two runs with the same
arguments."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "contig_h16", "--variants", "4000"]


def _run(out_dir):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *ARGS, "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_its_dumped_outputs(tmp_path):
    d = _run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert not {"roofline", "value_end_to_end", "dropin_threads", "cpu_baseline", "cohort", "sampler", "viterbi"} & d.keys()
    _run(tmp_path / "b")
    names = sorted(p.name for p in (tmp_path / "a").glob("*.npy"))
    assert "posterior.npy" in names and names == sorted(p.name for p in (tmp_path / "b").glob("*.npy"))
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), n
        assert np.isfinite(x).all(), n
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=0, err_msg=n)
    # a chain shorter than the sample is dumped whole; the posteriors of a variant are its normalised likelihoods
    a = tmp_path / "a"
    assert np.array_equal(np.load(a / "variant.npy"), np.arange(4000))
    post = np.load(a / "posterior.npy")
    assert np.isfinite(post).all() and (post >= 0).all() and (post <= 1 + 1e-12).all()
    assert np.load(a / "kept.npy").sum() > 0 and np.load(a / "n_columns.npy")[0] > 0
