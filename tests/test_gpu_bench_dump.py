"""GPU: a plain bench.py run (no --full) with --dump-outputs: the line holds
the headline figures only, --steps is the number of timed steps, and the file
written is the log_prob the timed path returned for the run's seeded rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_dumps_last_step_log_prob(hip_device, tmp_path):
    sys.path.insert(0, REPO)
    import bench
    from normalizingflow_amd import flush_status_checks

    rows, out = 5000, str(tmp_path / "dump")  # 5000: not a multiple of the kernels' 16-row tiles
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch", str(rows), "--dump-outputs", out]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True
    assert line["metric"] == bench.METRICS["c3"] and line["dtype"] == bench.DTYPE_FUSED
    assert line["ms_per_step"] > 0
    # value and ms_per_step say the same thing: rows per second of the timed steps
    # (ms_per_step is rounded to 1e-4 ms: 1 % of a 0.005 ms step, far below one launch)
    assert line["value"] == pytest.approx(rows / (line["ms_per_step"] * 1e-3), rel=1e-2)
    # what --full adds is not computed
    assert line["parity"] is None and line["roofline"] is None and line["cpu_baseline"] is None
    assert line["kernels"] == {} and "strong" not in line

    assert sorted(os.listdir(out)) == ["log_prob.npy"]
    lp = np.load(os.path.join(out, "log_prob.npy"))
    assert lp.dtype == np.float32 and lp.shape == (rows,)
    # the same rows and weights here: rank 0 draws x from a device generator seeded 0
    model, _, _ = bench.build_model("c3", hip_device)
    x = bench.make_x("c3", rows, torch.Generator(device=hip_device).manual_seed(0), hip_device)
    with torch.no_grad():
        ref = model.log_prob(x)
    torch.cuda.synchronize()
    flush_status_checks()
    assert np.array_equal(lp, ref.cpu().numpy())
