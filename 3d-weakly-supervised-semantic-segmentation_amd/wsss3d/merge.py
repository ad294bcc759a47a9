"""Batch assembly on the device.

`trainMerge` / `valMerge` (`dataset/data.py:135-238, 256-310`) run per batch
in the reference's DataLoader workers on the CPU; once the encoder step is on
the GPU that collation becomes the bottleneck.  Here the raw scenes stay in
HBM and `msp_merge` does the per-point work (rotation/scale, random offset,
crop, `.long()`, batch column, colour shift, scene labels, batch offsets) in
one pass; only the data-independent random draws come from the host, drawn
exactly as the numpy restatement (`wsss3d/synthetic.py: train_params,
val_params`) draws them, so both paths produce the same batch.

Subcloud training (`label: subcloud`, `dataset/data.py:69-125`; restated in
`wsss3d/subcloud.py`) cuts ~18 balls out of every room.  Here the balls are
never materialised: `SubcloudPool` draws the anchors on the host, counts
their members on the device (`msp_ball_count`) and keeps a list of
(scene, centre); `train_merge_subcloud_gpu` assembles a batch of such samples
with `msp_merge_ball`, the same kernels with the ball test fused in.
"""
from __future__ import annotations

import numpy as np
import torch

from sparseconvnet import _lib
from sparseconvnet._lib import call, ptr

from .edict import EasyDict
from .subcloud import anchor_noise, anchors_from_extrema
from .synthetic import NUM_CLASSES, train_params, val_params


class DeviceScenes:
    """Raw scenes resident in HBM: concatenated xyz / rgb (f32) and labels
    (int64), with the per-scene point ranges."""

    def __init__(self, scenes, device="cuda"):
        sizes = [len(a) for a, _, _ in scenes]
        self.start = [0]
        for n in sizes:
            self.start.append(self.start[-1] + n)
        self.max_points = max(sizes) if sizes else 0
        dev = torch.device(device)
        self.xyz = torch.from_numpy(np.concatenate([a for a, _, _ in scenes]).astype(np.float32)).to(dev)
        self.rgb = torch.from_numpy(np.concatenate([b for _, b, _ in scenes]).astype(np.float32)).to(dev)
        self.labels = torch.from_numpy(np.concatenate([c for _, _, c in scenes]).astype(np.int64)).to(dev)
        self.start_dev = torch.tensor(self.start, dtype=torch.int64, device=dev)
        self.device = dev

    def __len__(self):
        return len(self.start) - 1


def _param_tensors(params, dev):
    """The per-sample draws (rot, c1, c2, u1, u2, shift) as the device arrays msp_merge reads."""
    B = len(params)
    rot = torch.tensor(np.stack([p[0] for p in params]).reshape(B, 9), dtype=torch.float64, device=dev)
    c1 = torch.tensor(np.stack([p[1] for p in params]), dtype=torch.float64, device=dev)
    c2 = torch.tensor(np.stack([p[2] for p in params]), dtype=torch.float64, device=dev)
    u1 = torch.tensor(np.stack([p[3] for p in params]), dtype=torch.float64, device=dev)
    u2 = torch.tensor(np.stack([p[4] for p in params]), dtype=torch.float64, device=dev)
    shift = torch.tensor(np.stack([p[5] for p in params]), dtype=torch.float32, device=dev)
    return rot, c1, c2, u1, u2, shift


def _merge(sc: DeviceScenes, params, mode, full_scale, point_id_base=0):
    B = len(sc)
    dev = sc.device
    rot, c1, c2, u1, u2, shift = _param_tensors(params, dev)
    P = sc.start[-1]
    coords = torch.empty((max(P, 1), 4), dtype=torch.int64, device=dev)
    feats = torch.empty((max(P, 1), 3), dtype=torch.float32, device=dev)
    labels = torch.empty(max(P, 1), dtype=torch.int64, device=dev)
    ids = torch.empty(max(P, 1), dtype=torch.int64, device=dev) if mode == 1 else None
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    scene_labels = torch.empty((B, NUM_CLASSES), dtype=torch.float32, device=dev)
    wsb = int(_lib.query("msp_merge_workspace_size", B, _lib.I64(sc.max_points)))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    call("msp_merge", ptr(sc.xyz), ptr(sc.rgb), ptr(sc.labels), ptr(sc.start_dev), B, sc.max_points, mode,
         float(full_scale), ptr(rot), ptr(c1), ptr(c2), ptr(u1), ptr(u2), ptr(shift), NUM_CLASSES, ptr(coords),
         ptr(feats), ptr(labels), ptr(ids), int(point_id_base), ptr(offsets), ptr(scene_labels), ptr(ws), wsb,
         _lib.stream(dev))
    off = offsets.tolist()  # the one host read: batch_offsets is a python list in the reference
    n = off[-1]
    return coords[:n], feats[:n], labels[:n], (ids[:n] if ids is not None else None), off, scene_labels


def train_merge_gpu(sc: DeviceScenes, scale: float, full_scale: int = 4096, seed: int = 0):
    """Device `trainMerge`: EasyDict(x=EasyDict(coords, feature, batch_offsets),
    y_orig, y) like the reference's batch (`dataset/data.py:224-238`, point-cloud
    part); bitwise equal to wsss3d.synthetic.train_merge on the same scenes."""
    params = [train_params(scale, seed, i) for i in range(len(sc))]
    coords, feats, labels, _, off, sl = _merge(sc, params, 0, full_scale)
    return EasyDict(x=EasyDict(coords=coords, feature=feats, batch_offsets=off), y_orig=labels, y=sl)


def val_merge_gpu(sc: DeviceScenes, scale: float, full_scale: int = 4096, seed: int = 0, point_id_base=0):
    """Device `valMerge` (`dataset/data.py:256-310`): coords, feats, labels and
    the ids of the kept points (offset by point_id_base, the reference's
    valOffsets[i] for the first scene)."""
    params = []
    for i in range(len(sc)):
        m, _, c2, u1, u2, shift = val_params(scale, seed, i)
        params.append((m, np.full(3, full_scale / 2), c2, u1, u2, shift))
    coords, feats, labels, ids, off, sl = _merge(sc, params, 1, full_scale, point_id_base)
    return EasyDict(x=EasyDict(coords=coords, feature=feats), y_orig=labels, y=sl.long(), point_ids=ids,
                    batch_offsets=off)


class SubcloudPool:
    """The training list of `label: subcloud` (`dataset/data.py:89-125`) over scenes resident in HBM.

    The anchors of every scene are drawn on the host from the scene's extrema (computed on the device, read back
    in one copy) exactly as `wsss3d.subcloud.subcloud_anchors` draws them; `msp_ball_count` counts the members
    of every anchor in one launch and the counts are read back once.  Keeps

      entries  [(scene_idx, anchor_idx, count)] of the anchors with count >= min_points, scene-then-anchor order
      centres  (A, 3) f64 on the device, every anchor of every scene (anchor_start[s] + anchor_idx)
      counts   list of int64 arrays, the member count of every anchor per scene
    """

    def __init__(self, device_scenes: DeviceScenes, in_radius, min_points: int = 1000, seed: int = 0):
        if min_points < 1:
            raise ValueError(f"SubcloudPool: min_points must be >= 1 (got {min_points}); an empty ball is no sample")
        if not in_radius > 0:
            raise ValueError(f"SubcloudPool: in_radius must be positive (got {in_radius})")
        sc = device_scenes
        if len(sc) < 1:
            raise ValueError("SubcloudPool: no scenes")
        self.scenes, self.in_radius, self.min_points, self.seed = sc, in_radius, int(min_points), seed
        self.r2 = float(in_radius) * float(in_radius)
        dev = sc.device
        ext = torch.stack([torch.cat([sc.xyz[s0:s1].amin(0), sc.xyz[s0:s1].amax(0)])
                           for s0, s1 in zip(sc.start[:-1], sc.start[1:])]).cpu().numpy()
        centres, self.anchor_start = [], [0]
        for idx, e in enumerate(ext):
            anchors = anchors_from_extrema(e[:3], e[3:], in_radius)
            centres.append(anchors + anchor_noise(len(anchors), in_radius, seed, idx).astype(anchors.dtype))
            self.anchor_start.append(self.anchor_start[-1] + len(anchors))
        self.centres_host = np.concatenate(centres, 0)
        self.centres = torch.from_numpy(self.centres_host).to(dev)
        astart = torch.tensor(self.anchor_start, dtype=torch.int64, device=dev)
        counts = torch.empty(self.anchor_start[-1], dtype=torch.int64, device=dev)
        call("msp_ball_count", ptr(sc.xyz), ptr(sc.start_dev), len(sc), sc.max_points, ptr(self.centres),
             ptr(astart), self.r2, ptr(counts), _lib.stream(dev))
        counts = counts.cpu().numpy()
        self.counts = [counts[a0:a1] for a0, a1 in zip(self.anchor_start[:-1], self.anchor_start[1:])]
        self.entries = [(idx, k, int(n)) for idx, c in enumerate(self.counts) for k, n in enumerate(c)
                        if n >= self.min_points]

    def __len__(self):
        return len(self.entries)

    def centre(self, i):
        """Centre (3,) f64 of kept ball i."""
        idx, k, _ = self.entries[i]
        return self.centres_host[self.anchor_start[idx] + k]


def train_merge_subcloud_gpu(pool: SubcloudPool, indices, scale: float, full_scale: int = 4096, seed: int = 0):
    """Device `trainMerge` for the balls pool.entries[i], i in indices: the EasyDict of `train_merge_gpu` plus
    point_ids (each row's index into the pool's concatenated scenes); bitwise equal to
    wsss3d.subcloud.train_merge_subcloud on the same (scene, centre) entries."""
    sc, dev = pool.scenes, pool.scenes.device
    indices = list(indices)
    B = len(indices)
    if B < 1:
        raise ValueError("train_merge_subcloud_gpu: empty batch")
    rot, c1, c2, u1, u2, shift = _param_tensors([train_params(scale, seed, b) for b in range(B)], dev)
    scene_of = torch.tensor([pool.entries[i][0] for i in indices], dtype=torch.int32, device=dev)
    centre = torch.from_numpy(np.stack([pool.centre(i) for i in indices])).to(dev)
    cap = max(sum(pool.entries[i][2] for i in indices), 1)  # the balls' members, not the scenes' points
    coords = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    feats = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    labels = torch.empty(cap, dtype=torch.int64, device=dev)
    ids = torch.empty(cap, dtype=torch.int64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    scene_labels = torch.empty((B, NUM_CLASSES), dtype=torch.float32, device=dev)
    wsb = int(_lib.query("msp_merge_ball_workspace_size", B, _lib.I64(sc.max_points)))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    call("msp_merge_ball", ptr(sc.xyz), ptr(sc.rgb), ptr(sc.labels), ptr(sc.start_dev), B, sc.max_points, 0,
         float(full_scale), ptr(rot), ptr(c1), ptr(c2), ptr(u1), ptr(u2), ptr(shift), NUM_CLASSES, ptr(coords),
         ptr(feats), ptr(labels), ptr(ids), 0, ptr(offsets), ptr(scene_labels), ptr(ws), wsb, ptr(scene_of),
         ptr(centre), pool.r2, _lib.stream(dev))
    off = offsets.tolist()  # the one host read, as in _merge
    n = off[-1]
    return EasyDict(x=EasyDict(coords=coords[:n], feature=feats[:n], batch_offsets=off), y_orig=labels[:n],
                    y=scene_labels, point_ids=ids[:n])
