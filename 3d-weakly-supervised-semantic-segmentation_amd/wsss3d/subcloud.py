"""Subcloud-level training samples (`label: subcloud, in_radius: 2`), restated in numpy.

In this mode of the reference a training sample is a ball of radius `in_radius` cut out of a scene
(`dataset/data.py:28,35-36,63-64,69-125`): anchors lie on a grid over the scene's bounding box (`get_anchors`,
`:69-87`) with Gaussian noise of sigma in_radius/10 added (`:106-108`), a `KDTree.query_radius` is run per anchor
(`:109`), balls with fewer than 1000 points are dropped (`:111-112`) and each remaining ball becomes one entry of
the training list, which `trainMerge` then treats like a scene (`:135-238`): its weak label is the set of classes
present inside the ball (`:188-191`).

This module is the specification that the device path (wsss3d/merge.py: SubcloudPool, train_merge_subcloud_gpu;
csrc/msp_merge.hip: msp_ball_count, msp_merge_ball) reproduces bit for bit.  Membership of point i in the ball
of centre c is `query_radius`'s reduced-distance test for the Euclidean metric,

    d2 = ((dx*dx + dy*dy) + dz*dz) <= r*r,    dx = float64(x_i) - c_x,

every product and sum rounded separately in fp64, r*r formed once on the host.

Two deliberate deviations from the reference:

* the members of a ball are taken in ASCENDING POINT INDEX.  sklearn returns them in tree order, which is
  unspecified; the network depends on the order only through the summation order of the mode-4 average of points
  that share a voxel;
* the KDTree pickle stored beside each scene is not used: the test above is evaluated for every point of the
  scene, so no tree (and no sklearn) is needed.

Randomness is numpy-seeded per scene like `train_params`, so the host and the device path see the same anchors.
"""
from __future__ import annotations

import numpy as np

from .synthetic import NUM_CLASSES, _place, train_params, transform


def anchors_from_extrema(lo, hi, in_radius):
    """`get_anchors` (`dataset/data.py:77-87`) from the scene's float32 extrema lo, hi (3,): per axis
    floor((max - min) / in_radius) + 1 steps (float32 arithmetic, as numpy does on float32 scalars) and
    np.linspace(min, max, steps); x outermost, z innermost.  Returns (A, 3) float64."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    axes = []
    for j in range(3):
        steps = np.floor((hi[j] - lo[j]) / np.float32(in_radius)) + 1
        axes.append(np.linspace(lo[j], hi[j], int(steps)))
    return np.array([[x, y, z] for x in axes[0] for y in axes[1] for z in axes[2]], dtype=np.float64)


def get_anchors(points, in_radius):
    """`get_anchors` (`dataset/data.py:69-87`) of one scene's float32 coordinates (N, 3)."""
    points = np.asarray(points, np.float32)
    return anchors_from_extrema(points.min(0), points.max(0), in_radius)


def anchor_noise(n_anchors, in_radius, seed, scene_idx):
    """The noise of `data.py:107` for scene scene_idx: data-independent apart from the anchor count."""
    rng = np.random.RandomState(3000 + seed * 997 + scene_idx)
    return rng.normal(scale=in_radius / 10, size=(n_anchors, 3))


def subcloud_anchors(points, in_radius, seed, scene_idx):
    """The ball centres of one scene (`data.py:106-108`), float64 (A, 3)."""
    anchors = get_anchors(points, in_radius)
    return anchors + anchor_noise(len(anchors), in_radius, seed, scene_idx).astype(anchors.dtype)


def ball_members(points, centre, in_radius):
    """Boolean membership (N,) of the ball of `centre`: the test of the module docstring."""
    a = np.asarray(points).astype(np.float64)
    c = np.asarray(centre, np.float64)
    r2 = float(in_radius) * float(in_radius)
    dx, dy, dz = a[:, 0] - c[0], a[:, 1] - c[1], a[:, 2] - c[2]
    return ((dx * dx + dy * dy) + dz * dz) <= r2


def subcloud_counts(scenes, in_radius, seed=0):
    """Member count of every anchor, per scene: list of int64 arrays."""
    out = []
    for idx, (a, _, _) in enumerate(scenes):
        centres = subcloud_anchors(a, in_radius, seed, idx)
        out.append(np.array([int(ball_members(a, c, in_radius).sum()) for c in centres], np.int64))
    return out


def subcloud_list(scenes, in_radius, min_points=1000, seed=0):
    """The training list (`data.py:110-125`): [(scene_idx, anchor_idx, centre (3,) f64, count)] of the anchors
    with count >= min_points, in scene-then-anchor order."""
    out = []
    for idx, (a, _, _) in enumerate(scenes):
        for k, c in enumerate(subcloud_anchors(a, in_radius, seed, idx)):
            n = int(ball_members(a, c, in_radius).sum())
            if n >= min_points:
                out.append((idx, k, c, n))
    return out


def train_merge_subcloud(scenes, entries, scale: float, full_scale: int = 4096, seed: int = 0, in_radius=2):
    """`trainMerge` for a batch whose sample b is the ball entries[b] = (scene_idx, centre) of radius in_radius
    (default: the shipped subcloud configs' `in_radius: 2`):
    crops a, b, c to the ball's members (ascending point index), then exactly `train_merge` with
    train_params(scale, seed, b).  Returns train_merge's dict plus point_ids: each kept row's index inside its
    scene, offset by the scene's start in the concatenation of `scenes`."""
    start = np.concatenate([[0], np.cumsum([len(a) for a, _, _ in scenes])])
    locs, feats, labels, scene_labels, point_ids = [], [], [], [], []
    batch_offsets = [0]
    for idx, (scene_idx, centre) in enumerate(entries):
        a, b, c = scenes[scene_idx]
        members = np.nonzero(ball_members(a, centre, in_radius))[0]
        a, b, c = a[members], b[members], c[members]
        rot, c1, c2, u1, u2, shift = train_params(scale, seed, idx)
        if len(a):
            p, keep = _place(transform(a, rot, c1, c2), u1, u2, full_scale, "train")
        else:
            p, keep = np.zeros((0, 3)), np.zeros(0, bool)
        cc = c[keep]
        sl = np.zeros(NUM_CLASSES, np.float32)
        u = np.unique(cc)
        sl[u[u >= 0]] = 1.0
        locs.append(np.concatenate([p[keep].astype(np.int64), np.full((int(keep.sum()), 1), idx, np.int64)], 1))
        feats.append(b[keep] + shift)
        labels.append(cc)
        scene_labels.append(sl)
        point_ids.append(members[keep] + start[scene_idx])
        batch_offsets.append(batch_offsets[-1] + int(keep.sum()))
    return dict(coords=np.concatenate(locs, 0), feats=np.concatenate(feats, 0).astype(np.float32),
                batch_offsets=batch_offsets, labels=np.concatenate(labels, 0),
                scene_labels=np.stack(scene_labels, 0), point_ids=np.concatenate(point_ids, 0).astype(np.int64))
