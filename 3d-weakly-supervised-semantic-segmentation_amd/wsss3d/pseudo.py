"""The pseudo-label stage on the device (`pseudoLabelGeneration.py:46-59`, `utils/stats.py:5-55`,
`train.py:73-74` with `utils/loss.py:29-33`).

The reference labels the training points with the trained model

    logits = model(batch['x'])                                           # (N, 20) per-point logits
    pseudo_labels, num = get_pseudo_labels(logits, scene_label, batch_offsets, threshold)
    correct, total = assess_label_quality(pseudo_labels, batch['y_orig'])
    store_pseudo_label(pseudo_labels, scene_names, batch_offsets, path)

and then trains on those labels with the point branch of `Classification`.  Here the labelling is one launch
(`msp_pseudo_labels`: mask, normalise, sigmoid, max, threshold, quality counts, per-class confusion) that
leaves its input untouched, `PseudoLabelPass` keeps a pass's counts on the device and reads them once, and
`point_cross_entropy` is the loss without the boolean gather, so the pseudo-label training step can be
captured into a graph like every other training configuration.

Deviation from the reference, on purpose: a row with a non-finite logit is left unlabelled (-100) and not
counted; `utils/stats.py` gives such a row whatever NaN comparisons happen to produce.
"""
from __future__ import annotations

import os

import torch

from sparseconvnet import ops

from .registry import LOSS_REGISTRY
from .synthetic import NUM_CLASSES

IGNORE = -100


def _offsets(batch_offsets, n_rows, device):
    """(B + 1,) int64 device tensor from the reference's list (checked on the host, where it lives) or from a
    tensor (taken as it is: a device tensor is not read back)."""
    if torch.is_tensor(batch_offsets):
        return batch_offsets.to(device=device, dtype=torch.int64).contiguous()
    offs = [int(o) for o in batch_offsets]
    if len(offs) < 2 or offs[0] != 0 or offs[-1] != n_rows or any(a > b for a, b in zip(offs, offs[1:])):
        raise ValueError(f"batch_offsets {offs} do not partition {n_rows} rows")
    return torch.tensor(offs, dtype=torch.int64, device=device)


def get_pseudo_labels(logits, scene_label, batch_offsets, threshold=0.5):
    """`utils/stats.py:24-42`: (pseudo_labels (N,) int64 with -100 below the threshold, number of labels as a
    0-dim device tensor).  `logits` is not modified (the reference multiplies it by the scene mask in place)."""
    off = _offsets(batch_offsets, logits.size(0), logits.device)
    labels, _, counts = ops.pseudo_labels(logits.detach(), scene_label.to(torch.float32), off, threshold)
    return labels, counts[0]


def assess_label_quality(pseudo_labels, labels):
    """`utils/stats.py:44-48`: (correct, total) over the labelled points, as 0-dim tensors on the labels' device
    (no boolean gather, no host read)."""
    mask = pseudo_labels != IGNORE
    return ((pseudo_labels == labels) & mask).sum(), mask.sum()


def store_pseudo_label(pseudo_labels, scene_names, batch_offset, path, suffix="_pseudo_label.pth"):
    """`utils/stats.py:50-55`: one `<scene><suffix>` file per scene holding its slice of the labels (CPU int64,
    one device-to-host copy for the batch)."""
    host = pseudo_labels.detach().cpu()
    offs = batch_offset.tolist() if torch.is_tensor(batch_offset) else list(batch_offset)
    for b, scene_name in enumerate(scene_names):
        torch.save(host[int(offs[b]):int(offs[b + 1])].clone(), os.path.join(path, scene_name + suffix))


class PseudoLabelPass:
    """The body of `pseudoLabelGeneration.py:46-59` for a whole pass over the training set: `add()` labels one
    batch and accumulates {labelled, correct, rows} and the (label, gt) confusion on the device; `summary()` is
    the pass's single host read."""

    def __init__(self, device, n_classes: int = NUM_CLASSES, threshold: float = 0.5):
        self.threshold = float(threshold)
        self.counts = torch.zeros(3, dtype=torch.int64, device=device)
        self.confusion = torch.zeros((int(n_classes), int(n_classes)), dtype=torch.int64, device=device)

    def add(self, logits, scene_label, batch_offsets, y_orig=None, threshold=None):
        """Label one batch; returns its pseudo labels (device).  y_orig: the batch's ground truth (N,) int64 with
        -100 for unannotated points, or None (then nothing is counted as correct)."""
        off = _offsets(batch_offsets, logits.size(0), logits.device)
        gt = None if y_orig is None else y_orig.to(device=logits.device, dtype=torch.int64)
        labels, _, _ = ops.pseudo_labels(logits.detach(), scene_label.to(torch.float32), off,
                                         self.threshold if threshold is None else threshold, gt=gt,
                                         counts=self.counts, confusion=None if gt is None else self.confusion)
        return labels

    def summary(self):
        """One host read: counts, labelled share, precision (correct / labelled) and the per-class precision
        (diagonal over the row sums of the confusion; NaN for a class no labelled point carries)."""
        host = torch.cat([self.counts, self.confusion.flatten()]).cpu()
        labelled, correct, rows = (int(v) for v in host[:3])
        conf = host[3:].view_as(self.confusion).double()
        per_class = conf.diagonal() / conf.sum(1)
        nan = float("nan")
        return {"labelled": labelled, "correct": correct, "rows": rows,
                "labelled_share": labelled / rows if rows else nan,
                "precision": correct / labelled if labelled else nan,
                "class_precision": per_class.tolist(), "confusion": conf.long()}


def point_cross_entropy(logits, labels, return_counts=False):
    """`utils/loss.py:29-33` (`F.cross_entropy(logits[keep], labels[keep])`, keep = labels != -100) as one fused
    device loss with no host read in forward or backward.  No kept row: NaN loss, zero gradient.  With
    return_counts also (n_kept, n_bad) as 0-dim device tensors; n_bad counts labels that are neither -100 nor a
    class index (ignored, where torch's gather would fault)."""
    loss, n_kept, n_bad = ops.PointCrossEntropyFunction.apply(logits, labels)
    return (loss, n_kept, n_bad) if return_counts else loss


def voxel_point_cross_entropy(x, weight, bias, labels, level, rules, n_scenes, return_counts=False):
    """The training tail on pseudo labels (`models/MultiLabelContrastive.py:88-94` with `utils/loss.py:29-33`)
    from the level-0 voxel rows x (V, C_in) of an encoder, before its OutputLayer: with the per-point logits
    logits[p] = weight x[v(p)] + bias, returns (per-scene mean logits (B, C), point_cross_entropy(logits, labels))
    without forming the (N, C) logits or their gradient (ops.VoxelCrossEntropyFunction).  level / rules: the
    level-0 `Level` and the `InputRules` of the batch's metadata; scene b must be the points of batch id b
    (`InputRules.scene_ranges_match`).  With return_counts also (n_kept, n_bad) as 0-dim device tensors."""
    scene, loss, n_kept, n_bad = ops.VoxelCrossEntropyFunction.apply(x, weight, bias, labels, level, rules,
                                                                     int(n_scenes))
    return (scene, loss, n_kept, n_bad) if return_counts else (scene, loss)


@LOSS_REGISTRY.register()
def PointClassification(logits: torch.Tensor, labels: torch.Tensor):
    """The point branch of `Classification` for training on pseudo labels (train.py:73-74), capturable."""
    return point_cross_entropy(logits, labels)
