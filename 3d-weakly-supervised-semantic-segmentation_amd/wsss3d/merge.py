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

Elastic distortion (`elastic_deformation: True`, `dataset/data.py:171-173`; restated in `wsss3d/elastic.py`):
`elastic=True` on the two training calls displaces every sample by two smooth random fields between the rotation
and the offset (`msp_merge_elastic`).  The noise grids are drawn on the host at a shape bounded from the scene's
`abs_extrema` and the rotation, so nothing is read back in the middle of a batch.
"""
from __future__ import annotations

import numpy as np
import torch

from sparseconvnet import _lib
from sparseconvnet._lib import call, ptr

from .edict import EasyDict
from .elastic import ball_abs_extrema, sample_elastic_params
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
        self._abs_extrema = None

    def __len__(self):
        return len(self.start) - 1

    @property
    def abs_extrema(self):
        """Per-scene max |raw xyz| (n_scenes, 3) f64 on the host (zeros for an empty scene): the bound the elastic
        noise grids are sized from.  Computed on the device at the first use, one read-back."""
        if self._abs_extrema is None:
            zero = torch.zeros(3, dtype=torch.float32, device=self.device)
            ext = torch.stack([self.xyz[s0:s1].abs().amax(0) if s1 > s0 else zero
                               for s0, s1 in zip(self.start[:-1], self.start[1:])])
            self._abs_extrema = ext.cpu().numpy().astype(np.float64)
        return self._abs_extrema


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


def _field_tensors(eparams, field, dev):
    """Field `field`'s raw noise of every sample as msp_merge_elastic reads it: (noise f32 flat, cap (B,3) int32,
    cell_off (B+1,) int64) on the device and the cell total."""
    caps = np.stack([np.asarray(e["cap%d" % field], np.int64) for e in eparams])
    off = np.concatenate([[0], np.cumsum(caps.prod(1))]).astype(np.int64)
    flat = []
    for e, cap in zip(eparams, caps):
        for n in e["noise%d" % field]:
            if n.shape != tuple(cap) or n.dtype != np.float32:
                raise ValueError(f"elastic noise of shape {n.shape} / {n.dtype}, expected {tuple(cap)} float32")
            flat.append(n.ravel())
    noise = torch.from_numpy(np.concatenate(flat)).to(dev)
    return noise, torch.from_numpy(caps.astype(np.int32)).to(dev), torch.from_numpy(off).to(dev), int(off[-1])


def merge_elastic_gpu(sc: DeviceScenes, params, eparams, full_scale, scene_of=None, centres=None, r2=0.0,
                      capacity=None):
    """The lower-level call behind `elastic=True`: `trainMerge` with the draws params[b] (`train_params`' tuple)
    and eparams[b] (`wsss3d.elastic.elastic_params`' dict) of sample b.  Sample b is scene b, or with scene_of
    (list of int) and centres ((B,3) f64) the ball of squared radius r2 around centres[b] in scene scene_of[b].
    All samples share eparams[0]'s gran / mag.  capacity: output rows (default: all points of the scenes).
    Returns (coords, feats, labels, point_ids, batch_offsets list, scene_labels); raises RuntimeError when a
    grid turned out smaller than the data needs (status != 0)."""
    dev = sc.device
    B = len(params)
    if B < 1 or len(eparams) != B:
        raise ValueError("merge_elastic_gpu: one params and one eparams entry per sample")
    e0 = eparams[0]
    for e in eparams:
        if any(e[k] != e0[k] for k in ("gran1", "mag1", "gran2", "mag2")):
            raise ValueError("merge_elastic_gpu: every sample of a batch has the same gran / mag")
    rot, c1, c2, u1, u2, shift = _param_tensors(params, dev)
    noise1, cap1, off1, n1 = _field_tensors(eparams, 1, dev)
    noise2, cap2, off2, n2 = _field_tensors(eparams, 2, dev)
    cells = max(n1, n2)
    balls = scene_of is not None
    if balls:
        scene_of_t = torch.tensor(list(scene_of), dtype=torch.int32, device=dev)
        centre_t = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float64)).to(dev)
    elif B != len(sc):
        raise ValueError("merge_elastic_gpu: whole scenes need one sample per scene")
    cap = max(int(capacity) if capacity is not None else sc.start[-1], 1)
    coords = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    feats = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    labels = torch.empty(cap, dtype=torch.int64, device=dev)
    ids = torch.empty(cap, dtype=torch.int64, device=dev)
    tail = torch.zeros(B + 2, dtype=torch.int64, device=dev)  # batch_offsets[B+1], then status in the low word
    scene_labels = torch.empty((B, NUM_CLASSES), dtype=torch.float32, device=dev)
    wsb = int(_lib.query("msp_merge_elastic_workspace_size", B, _lib.I64(sc.max_points), _lib.I64(cells)))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    call("msp_merge_elastic", ptr(sc.xyz), ptr(sc.rgb), ptr(sc.labels), ptr(sc.start_dev), B, sc.max_points, 0,
         float(full_scale), ptr(rot), ptr(c1), ptr(c2), ptr(u1), ptr(u2), ptr(shift), NUM_CLASSES, ptr(coords),
         ptr(feats), ptr(labels), ptr(ids), 0, ptr(tail), ptr(scene_labels), ptr(ws), wsb,
         ptr(scene_of_t) if balls else None, ptr(centre_t) if balls else None, float(r2), ptr(noise1), ptr(noise2),
         ptr(cap1), ptr(cap2), ptr(off1), ptr(off2), cells, int(e0["gran1"]), float(e0["mag1"]), int(e0["gran2"]),
         float(e0["mag2"]), tail.data_ptr() + 8 * (B + 1), _lib.stream(dev))
    *off, status = tail.tolist()  # the one host read: the offsets and the status word together
    if status:
        raise RuntimeError(f"msp_merge_elastic: status {status}: " +
                           ("a noise grid is smaller than its sample's extent (bb clamped to cap)" if status & 1
                            else "inconsistent cap / cell offsets"))
    n = off[-1]
    return coords[:n], feats[:n], labels[:n], ids[:n], off, scene_labels


def train_merge_gpu(sc: DeviceScenes, scale: float, full_scale: int = 4096, seed: int = 0, elastic: bool = False):
    """Device `trainMerge`: EasyDict(x=EasyDict(coords, feature, batch_offsets),
    y_orig, y) like the reference's batch (`dataset/data.py:224-238`, point-cloud
    part); bitwise equal to wsss3d.synthetic.train_merge on the same scenes.
    elastic (the config key `elastic_deformation`): the two elastic fields of `data.py:171-173` between the
    rotation and the offset; bitwise equal to wsss3d.elastic.train_merge_elastic."""
    params = [train_params(scale, seed, i) for i in range(len(sc))]
    if elastic:
        ext = sc.abs_extrema
        eparams = [sample_elastic_params(ext[i], params[i][0], scale, seed, i) for i in range(len(sc))]
        coords, feats, labels, _, off, sl = merge_elastic_gpu(sc, params, eparams, full_scale)
        return EasyDict(x=EasyDict(coords=coords, feature=feats, batch_offsets=off), y_orig=labels, y=sl)
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


def train_merge_subcloud_gpu(pool: SubcloudPool, indices, scale: float, full_scale: int = 4096, seed: int = 0,
                             elastic: bool = False):
    """Device `trainMerge` for the balls pool.entries[i], i in indices: the EasyDict of `train_merge_gpu` plus
    point_ids (each row's index into the pool's concatenated scenes); bitwise equal to
    wsss3d.subcloud.train_merge_subcloud on the same (scene, centre) entries.
    elastic (`elastic_deformation`): as in `train_merge_gpu`, the grids sized from min(scene extrema, |centre| +
    in_radius); bitwise equal to wsss3d.elastic.train_merge_subcloud_elastic."""
    sc, dev = pool.scenes, pool.scenes.device
    indices = list(indices)
    B = len(indices)
    if B < 1:
        raise ValueError("train_merge_subcloud_gpu: empty batch")
    if elastic:
        params = [train_params(scale, seed, b) for b in range(B)]
        scene_of = [pool.entries[i][0] for i in indices]
        centres = np.stack([pool.centre(i) for i in indices])
        ext = sc.abs_extrema
        eparams = [sample_elastic_params(ball_abs_extrema(ext[scene_of[b]], centres[b], pool.in_radius),
                                         params[b][0], scale, seed, b) for b in range(B)]
        coords, feats, labels, ids, off, sl = merge_elastic_gpu(
            sc, params, eparams, full_scale, scene_of, centres, pool.r2,
            capacity=sum(pool.entries[i][2] for i in indices))
        return EasyDict(x=EasyDict(coords=coords, feature=feats, batch_offsets=off), y_orig=labels, y=sl,
                        point_ids=ids)
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
