"""bench.py's plain run on the GPU, in a child process: it times exactly --steps steps, its line carries the headline fields and none of
the --full legs, and --dump-outputs writes the ids that the images of the LAST timed step got back from generate()."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    B, n_new, steps, warmup = 16, 8, 2, 1
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--n-new", str(n_new),
           "--images-per-gpu", str(B), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["unit"] == "tokens/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["metric"].startswith("decoded tokens/sec LLaVA-1.5-7B")
    assert line["ms_per_step"] > 0 and abs(line["value"] - B * n_new / (line["ms_per_step"] * 1e-3)) < 1e-3 * line["value"] + 0.05
    for k in ("roofline", "single_stream", "single_stream_two_sweep", "single_stream_nonempty_keep_sets", "determinism_check"):
        assert line[k] is None, k                                   # --full legs
    assert "cpu_baseline" not in line
    ids = np.load(out / "token_ids.npy")
    assert ids.dtype == np.float64 and ids.shape == (B, 32 + n_new)
    assert (ids == np.round(ids)).all() and ids.min() >= 0 and ids.max() < 32064
    # the rows are the prompts of the last timed step's images (batch `warmup + steps - 1`, image b = default_rng(batch * B + b)) + new ids
    sys.path.insert(0, ROOT)
    import bench
    last = warmup + steps - 1
    for b in range(B):
        want, _ = bench.synthetic_inputs(last * B + b, 32064, 32000)
        np.testing.assert_array_equal(ids[b, :32], want[0].numpy())
