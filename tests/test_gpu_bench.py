"""bench.py's plain line and --dump-outputs on the GPU: a small batch, run twice in fresh processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--records", "2000", "--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    """the plain run: the headline keys, exactly --steps timed steps, none of the --full legs; the dumped arrays are the last
    step's (totals = column sums of the counters, clean diagnostics, the rows' total), and a second process writes the
    same files"""
    d = _bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "ops/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert abs(d["value"] - d["config"]["ops_per_gpu"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("cpu_baseline", "e2e"):
        assert k not in d
    assert "allocation_spread" not in d["roofline"] and "extra_shapes_ms" not in d["roofline"]

    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in ("totals", "rows_sample", "counts", "diag", "t_row_off", "q_row_off", "rec_off"))
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["counts"].shape == (2000, 11) and (a["diag"] == -1).all()
    assert np.array_equal(a["totals"], a["counts"].sum(0))
    assert a["rec_off"][-1] == d["config"]["output_bytes_per_gpu"]
    assert a["rows_sample"].min() >= 0 and a["rows_sample"].max() <= 255 and a["rows_sample"].any()

    _bench(tmp_path / "b")
    for f in names:
        assert np.array_equal(np.load(tmp_path / "b" / f), a[f[:-4]]), f
