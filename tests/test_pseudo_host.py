"""Host side of the pseudo-label stage: argument validation of the new entry points without a GPU, the IoU
arithmetic against the fixture made by the reference's own utils/iou.py (tests/golden/make_pseudo_golden.py), and
the per-scene label files."""
import math
import os

import numpy as np
import pytest
import torch

from sparseconvnet import _lib
from wsss3d import LOSS_REGISTRY, store_pseudo_label
from wsss3d.evaluate import iou_from_confusion
from wsss3d.pseudo import PointClassification

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pseudo_labels.npz")


def test_argument_validation_without_gpu():
    lib = _lib.load()
    for C in (0, 65):
        rc = lib.msp_pseudo_labels(None, 10, C, None, None, 1, 0.5, None, None, None, None, None, None)
        assert rc == -1 and b"msp_pseudo_labels: C=" in lib.msp_last_error()
        rc = lib.msp_confusion(None, None, 10, C, None, None)
        assert rc == -1 and b"msp_confusion: C=" in lib.msp_last_error()
        rc = lib.msp_point_ce_fwd(None, 10, C, None, None, None, None, None, None, 1 << 20, None)
        assert rc == -1 and b"msp_point_ce_fwd: C=" in lib.msp_last_error()
        rc = lib.msp_point_ce_bwd(None, 10, C, None, None, None, None, None, None)
        assert rc == -1 and b"msp_point_ce_bwd: C=" in lib.msp_last_error()
    need = _lib.query("msp_point_ce_workspace_size", 10 ** 6)
    assert 0 < need <= 1 << 16 and _lib.query("msp_point_ce_workspace_size", 0) > 0
    rc = lib.msp_point_ce_fwd(None, 10 ** 6, 20, None, None, None, None, None, None, need - 1, None)
    assert rc == -1 and b"workspace too small" in lib.msp_last_error()
    rc = lib.msp_pseudo_labels(None, 10, 20, None, None, 0, 0.5, None, None, None, None, None, None)
    assert rc == -1 and b"B=0" in lib.msp_last_error()
    with pytest.raises(RuntimeError, match="msp_confusion"):
        _lib.call("msp_confusion", None, None, -1, 20, None, None)
    assert LOSS_REGISTRY.get("PointClassification")[0] is PointClassification


def test_iou_from_confusion_matches_the_reference():
    z = np.load(GOLDEN)
    ious, mean_iou = iou_from_confusion(z["confusion"])
    assert ious.shape == (20,) and ious.dtype == np.float64
    assert abs(mean_iou - float(z["mean_iou"])) <= 1e-12
    ious_t, mean_t = iou_from_confusion(torch.from_numpy(z["confusion"]))
    assert mean_t == mean_iou and np.array_equal(ious_t, ious)
    conf = z["confusion"]
    tp = np.diag(conf)
    assert np.allclose(ious, tp / (conf.sum(0) + conf.sum(1) - tp), rtol=0, atol=1e-15)


def test_iou_of_an_empty_class_is_nan():
    conf = np.zeros((20, 20), dtype=np.int64)
    conf[0, 0], conf[1, 0], conf[1, 1] = 3, 1, 4
    ious, mean_iou = iou_from_confusion(conf)
    assert ious[0] == 3 / 4 and ious[1] == 4 / 5
    assert np.isnan(ious[2:]).all() and math.isnan(mean_iou)


def test_store_pseudo_label_round_trip(tmp_path):
    labels = torch.tensor([3, -100, 7, 7, -100, 0, 19], dtype=torch.int64)
    names = ["scene0000_00", "scene0001_00", "scene0002_01"]
    offsets = [0, 3, 3, 7]
    store_pseudo_label(labels, names, offsets, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == [n + "_pseudo_label.pth" for n in names]
    for b, n in enumerate(names):
        back = torch.load(os.path.join(tmp_path, n + "_pseudo_label.pth"))
        assert back.dtype == torch.int64 and torch.equal(back, labels[offsets[b]:offsets[b + 1]])
    store_pseudo_label(labels, names[:1], torch.tensor(offsets), str(tmp_path), suffix=".pth")
    assert torch.equal(torch.load(os.path.join(tmp_path, "scene0000_00.pth")), labels[:3])
