"""GPU: bench.py's plain run -- exactly --steps timed steps, the headline line alone (the other sections are --full's), and
--dump-outputs writing the logits of the last timed step, the same as decode_lattice gives for the bench's seeded scene."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def test_bench_plain_run_times_exactly_steps_and_dumps_the_last_logits(tmp_path):
    nx = 64
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                          "--nx", str(nx), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 5 and res["timing"]["timed_steps"] == 5 and res["ms_per_step"] > 0
    assert res["unit"] == "query-points/s" and res["higher_is_better"] is True and res["dtype"] == "f16x3" and res["value"] > 0
    for key in ("exact_f32_kernel", "mesh_extract", "stages_ms", "sharded_scene", "train_step", "config3", "cpu_baseline"):
        assert key not in res, key
    got = np.load(tmp_path / "logits.npy")
    assert got.dtype == np.float32 and got.shape == (1, nx ** 3) and np.isfinite(got).all()

    from vtaco_amd.bench_util import build_scene
    dev = torch.device("cuda:0")
    scene = build_scene(0, dev)
    with torch.no_grad():
        ref = scene["model"].decoder.decode_lattice(scene["grid"], nx, box=1.1, precision="f16x3").cpu().numpy()
    assert float(np.abs(got - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))
