"""bench.py's command line on a small workload: a plain run times exactly --steps steps and reports nothing
that needs runs of its own, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    from wsss3d.synthetic import make_batch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "2", "--scale", "20", "--dump-outputs", str(out)],
                       cwd=root, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["unit"] == "active-voxels/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    # three timed steps over the two alternating batches (0, 1, 0): value x ms_per_step is their mean voxel count
    hb = [make_batch(2, 20, seed=k) for k in range(2)]
    v = [len(np.unique(b["coords"], axis=0)) for b in hb]
    assert d["value"] * d["ms_per_step"] * 1e-3 == pytest.approx((2 * v[0] + v[1]) / 3, rel=1e-9)
    for k in ("roofline", "roofline_families", "step_roofline", "cpu_baseline"):
        assert k not in d, k
    assert d["config"]["levels"] is None and d["config"]["fwd_multiply_adds"] is None

    assert sorted(os.listdir(out)) == ["grad_sample.npy", "logits.npy", "loss.npy", "param_sample.npy"]
    a = {n: np.load(out / (n + ".npy")) for n in ("loss", "logits", "grad_sample", "param_sample")}
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["loss"].shape == () and a["logits"].shape == (2, 20)
    assert a["grad_sample"].shape == a["param_sample"].shape and a["grad_sample"].ndim == 1
    assert 0 < a["grad_sample"].size <= 1 << 20 and np.abs(a["grad_sample"]).max() > 0
    # the dumped loss is the loss of the dumped logits on the last timed step's batch (step 2 -> batch 0)
    y = torch.from_numpy(hb[0]["scene_labels"])
    want = torch.nn.functional.multilabel_soft_margin_loss(torch.from_numpy(a["logits"]).double(), y.double())
    assert abs(float(a["loss"]) - want.item()) <= 1e-6 * max(1.0, abs(want.item()))
