"""bench.py's command line: what a plain run does, what --full adds, what --dump-outputs writes.

A plain run times its steps and prints the result line only; --full adds the measurements beside
the headline (extra steps, roofline, the reference's call loop, CPU baseline, MSE against it).
--dump-outputs DIR writes the last timed step's accumulator as DIR/accum.npy: with strong scaling
step s renders frame ids 1 + s*spp .. (s+1)*spp, so after W warm-up and K timed steps the image is
the sum over the frames of step W + K - 1, which must equal the oracle's sum over the same frame
ids bit for bit (the kernels and the oracle share the path's arithmetic).

The runs are small (64x48, 4 spp, depth 8, the default config's scene) and each is one process.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import oracle_render

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP, DEPTH = 64, 48, 4, 8
WARMUP, STEPS = 1, 2
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "value_primary_per_frame", "value_reference_loop", "reference_loop", "cpu_baseline",
             "mse_vs_oracle")


def _bench(cwd, *extra):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--width", str(W), "--height", str(H), "--spp", str(SPP), "--depth", str(DEPTH), *extra]
    p = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout  # one JSON result line
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    from optixpathtracer_amd import scenes

    out = _bench(tmp_path, "--dump-outputs", str(tmp_path / "dump"))
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["full"] is False
    assert out["unit"] == "Msamples/sec" and out["higher_is_better"] is True and out["dtype"] == "f32"
    # value and ms_per_step describe the same timed region (both are rounded in the line)
    rate = W * H * SPP / (out["ms_per_step"] / 1e3) / 1e6
    assert out["ms_per_step"] > 0 and abs(rate - out["value"]) <= 0.02 * out["value"] + 1e-3
    for k in FULL_ONLY:
        assert k not in out, k
    assert sorted(p.name for p in (tmp_path / "dump").iterdir()) == ["accum.npy"]
    img = np.load(tmp_path / "dump" / "accum.npy")
    assert img.dtype == np.float32 and img.shape == (H, W, 3)
    first = 1 + (WARMUP + STEPS - 1) * SPP
    ref, _ = oracle_render(scenes.make_scene("sphere_box_diffuse"), W, H, DEPTH, first, SPP)
    assert np.array_equal(img, ref.astype(np.float32))
    assert out["image"]["mean"] == pytest.approx(float(np.nanmean(img) / SPP), rel=1e-6)


def test_full_run_adds_the_other_measurements(tmp_path):
    out = _bench(tmp_path, "--full", "--cpu-baseline-seconds", "0.5", "--reference-loops", "8")
    assert out["full"] is True
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert out["roofline"]["kernel"] == "k_trace_pair" and out["roofline"]["launches"] > 0
    assert out["cpu_baseline"]["value"] > 0
    assert out["mse_vs_oracle"]["mse"] <= out["mse_vs_oracle"]["bar"]
