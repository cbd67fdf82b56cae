"""bench.py --dump-outputs: what the last timed step computed, written so that two builds compare output for output.

CPU: the writer (float32 .npy per array, a fixed seeded sample of an array beyond its share of the 64 MB cap).  GPU: two plain
runs with the same arguments write identical arrays, and a plain run times exactly --steps steps and carries none of --full's
legs.  bench.py runs in a child process: importing it here would set its HIP environment in the test process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_writer_caps_and_samples_the_same_elements(tmp_path):
    code = ("import sys, torch; sys.path.insert(0, %r); import bench\n"
            "bench.DUMP_BYTES = 4096\n"
            "big = torch.arange(3000, dtype=torch.float64).reshape(30, 100)\n"
            "small = torch.arange(6, dtype=torch.float32).reshape(2, 3)\n"
            "for d in sys.argv[1:]:\n"
            "    bench.dump_outputs(d, {'big': big, 'small': small})\n" % ROOT)
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    p = subprocess.run([sys.executable, "-c", code] + dirs, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    a = {n: np.load(os.path.join(dirs[0], n + ".npy")) for n in ("big", "small")}
    b = {n: np.load(os.path.join(dirs[1], n + ".npy")) for n in ("big", "small")}
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 4096
    np.testing.assert_array_equal(a["small"], np.arange(6, dtype=np.float32).reshape(2, 3))
    big = a["big"]
    assert big.shape == (4096 // 4 // 2,) and np.all(np.diff(big) > 0) and big.min() >= 0 and big.max() < 3000
    assert np.array_equal(big, np.round(big))           # elements of the array, not an interpolation
    for n in a:
        np.testing.assert_array_equal(a[n], b[n])


def _plain_run(out_dir):
    args = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--pre-warm-steps", "64", "--dump-outputs", out_dir]
    p = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_runs_are_reproducible_output_for_output(dev, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _plain_run(a)
    _plain_run(b)
    assert line["steps"] == 6 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"long_run", "roofline", "extra_legs", "cpu_baseline"} & set(line)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and {"theta.npy", "losses.npy", "depth.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
        total += x.nbytes
    assert total <= 64 << 20
