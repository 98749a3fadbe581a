"""bench.py's plain run (the headline read leg alone) and the files --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_results(tmp_path, oracle):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--workload", "c2small", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 4 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert (line["unit"], line["higher_is_better"], line["dtype"]) == ("MB/s", True, "u8")
    assert "compress_MBps" not in line and "cpu_baseline" not in line and "roofline" not in line  # behind --full
    rows, chunk = 2000, 10240
    nbytes = rows * chunk
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
    counters = np.load(out / "counters.npy")
    assert counters.dtype == np.float64 and list(counters) == [rows, nbytes, nbytes, 0, 0, 0]
    status = np.load(out / "row_status.npy")
    assert status.dtype == np.float32 and status.shape == (rows,) and (status == 0).all()
    digests = np.load(out / "row_digests.npy")
    want = np.frombuffer(oracle.blake3(gen.text(chunk)), np.uint8)  # every c2 row is the same chunk
    assert digests.dtype == np.float32 and digests.shape == (rows, 32) and (digests == want).all()
    sample = np.load(out / "decoded_bytes_sample.npy")
    pos = np.sort(np.random.default_rng(1).integers(0, nbytes, 1 << 22))
    assert sample.dtype == np.float32 and np.array_equal(sample, np.frombuffer(gen.text(chunk), np.uint8)[pos % chunk])
