"""Validation accumulation on the device (train.py:94-116).

The reference's eval loop is

    store = torch.zeros(valOffsets[-1], 20)
    for rep in range(1, 1 + val_reps):
        for batch in val_data_loader:
            predictions = model(batch['x'])                              # (N, 20) per-point logits
            store.index_add_(0, batch['point_ids'], predictions.cpu())   # train.py:107
    mean_iou = iou.evaluate(store.max(1)[1].numpy(), valLabels)

`PointLogitStore` keeps `store` in HBM: `add()` is the `index_add_` on the device (msp_index_add_rows,
bit-equal to the CPU loop for any ids, repeated ids included), so the per-batch device-to-host copy of
the (N, 20) predictions goes away; `cpu()` / `argmax()` hand the result to the reference's
`utils/iou.py` once per evaluation.  The predictions come from the heads' fused eval path
(heads.point_logits: the Linear on the voxel rows, no (N, C) feature tensor).

`confusion_matrix` / `iou_from_confusion` / `PointLogitStore.evaluate` are `utils/iou.py:19-53` with the
confusion counted on the device (msp_confusion): an evaluation moves the 20 x 20 counts to the host instead of
one label per point.
"""
from __future__ import annotations

import torch

import numpy as np

from sparseconvnet.ops import confusion_add, index_add_rows

from .synthetic import NUM_CLASSES


def confusion_matrix(pred, gt, n_classes: int = NUM_CLASSES, out=None):
    """`iou.confusion_matrix` (utils/iou.py:19-22) on the device: int64 (n_classes, n_classes) with
    [pred, gt] counted over the points whose gt >= 0.  `out`: an int64 matrix to accumulate into (several
    batches); a prediction outside [0, n_classes) is skipped.  Nothing is read back."""
    pred = pred.to(torch.int64)
    gt = gt.to(device=pred.device, dtype=torch.int64)
    if out is None:
        out = torch.zeros((int(n_classes), int(n_classes)), dtype=torch.int64, device=pred.device)
    return confusion_add(out, pred.reshape(-1), gt.reshape(-1))


def iou_from_confusion(conf):
    """Per-class IoU (float64 array) and their mean from a (C, C) confusion, with the arithmetic of
    `iou.get_iou` / `iou.evaluate` (utils/iou.py:24-45): tp / (tp + fp + fn) per class in float64, the mean as
    the running sum of iou / C.  A class with an empty denominator gives NaN (and so a NaN mean) where the
    reference raises a TypeError on `float('nan')[0]`."""
    c = conf.detach().cpu().numpy() if torch.is_tensor(conf) else np.asarray(conf)
    c = c.astype(np.int64)
    n = c.shape[0]
    ious = np.empty(n, dtype=np.float64)
    mean_iou = 0
    for i in range(n):
        tp = int(c[i, i])
        denom = int(c[i, :].sum()) + int(c[:, i].sum()) - tp
        ious[i] = float(tp) / denom if denom else float("nan")
        mean_iou += ious[i] / n
    return ious, float(mean_iou)


class PointLogitStore:
    """Device twin of train.py:96's `store = torch.zeros(valOffsets[-1], 20)`."""

    def __init__(self, n_points: int, device, n_classes: int = NUM_CLASSES):
        self.store = torch.zeros((int(n_points), int(n_classes)), dtype=torch.float32, device=device)

    def add(self, point_ids: torch.Tensor, predictions: torch.Tensor):
        """store.index_add_(0, point_ids, predictions) (train.py:107)."""
        index_add_rows(self.store, point_ids, predictions.detach())
        return self

    def argmax(self) -> torch.Tensor:
        """store.max(1)[1] (train.py:114)."""
        return self.store.max(1)[1]

    def cpu(self) -> torch.Tensor:
        return self.store.cpu()

    def evaluate(self, gt_labels: torch.Tensor, return_classes: bool = False):
        """`iou.evaluate(store.max(1)[1].numpy(), valLabels)` (train.py:114-115) -> mean IoU, with the confusion
        counted on the device: n_classes^2 integers go to the host instead of one label per point."""
        conf = confusion_matrix(self.argmax(), gt_labels.to(self.store.device), self.store.size(1))
        ious, mean_iou = iou_from_confusion(conf)
        return (mean_iou, ious) if return_classes else mean_iou
