"""A plain `bench.py` run: the headline line alone, EXACTLY --steps timed steps, and --dump-outputs writes what its timed
forward returned (compared here with the same seeded forward run in this process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["unit"] == "edges/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(line["config"]["E"] / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert "stress" not in line and "roofline" not in line and "cpu_baseline" not in line      # (--full only)
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["classified_edges_0", "latent_node_feats"]
    assert all(a.dtype == np.float32 for a in got.values())

    sys.path.insert(0, ROOT)
    import bench
    _, model, data = bench.setup_workload("s02", torch.device("cuda:0"))
    with torch.no_grad():
        want, want_h = model(data)
    torch.cuda.synchronize()
    w = want["classified_edges"][0].cpu().numpy()
    assert got["classified_edges_0"].shape == w.shape
    assert np.abs(got["classified_edges_0"] - w).max() <= 1e-5 * max(1.0, np.abs(w).max())
    h = want_h.cpu().numpy()
    assert np.abs(got["latent_node_feats"] - h).max() <= 1e-5 * max(1.0, np.abs(h).max())
