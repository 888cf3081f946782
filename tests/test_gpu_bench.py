"""A plain `bench.py` run on the GPU: set-up, warm-up, the timed steps, --dump-outputs and the headline line, and none of the
measurements that `--full` adds after the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_alone(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "8", "--warmup", "8",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["unit"] == "captions/s" and line["higher_is_better"] is True and line["dtype"] == "fp16"
    assert line["steps"] == 8 and line["warmup"] == 8 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(16 * 1e3 / line["ms_per_step"], rel=1e-9)
    assert not {"forward_sync", "pipelined_groups", "roofline", "stages", "vit_launch_160", "sync", "preprocess", "configs",
                "cpu_baseline"} & set(line)
    assert np.load(tmp_path / "trace_ids.npy").shape == (16, 30)
    assert np.load(tmp_path / "trace_capts.npy").shape[0] == 16
