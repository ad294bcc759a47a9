"""Elastic distortion of `trainMerge` (`elastic_deformation: True`), restated in numpy.

The reference distorts every training sample twice between the rotation and the random offset
(`dataset/data.py:171-173`): `elastic(a, 6*scale//50, 40*scale/50)` then `elastic(a, 20*scale//50, 160*scale/50)`
with `elastic` of `dataset/dataset_utils/data_processing.py:8-21`: three grids of Gaussian noise over the sample's
bounding box at a spacing of 2*gran voxels, blurred six times with a 3-tap box, interpolated trilinearly at every
point and added to it, times mag.

This module is the specification that the device path (csrc/msp_elastic.hip: msp_merge_elastic;
wsss3d/merge.py: `elastic=True`) follows operation by operation: fp64, every product and sum rounded
separately, in the order written here (as `synthetic.transform` does for the rotation).  No scipy at run time.

One deliberate deviation from the reference.  The reference draws `randn(*bb)` with bb computed from the data,
so the draw cannot be made before the points are transformed.  Here the grids are drawn at a data-independent
shape cap >= bb (`elastic_caps`, `elastic_cap2`) from a per-sample RandomState, and the field uses the
[:bb0, :bb1, :bb2] corner of the draw: the device path needs no read-back in the middle of a batch.  The blur
sees zeros beyond bb, never the drawn values there, so a field is exactly the reference's for the noise in its
corner.
"""
from __future__ import annotations

import numpy as np

from .subcloud import ball_members
from .synthetic import NUM_CLASSES, _place, train_params, transform

# the box weight as the reference holds it: float32(1)/float32(3), widened
BLUR_W = np.float64(np.float32(1) / np.float32(3))


def elastic_grans(scale):
    """(gran1, mag1, gran2, mag2) of `data.py:172-173` for `scale`; gran is a positive integer."""
    gran1, gran2 = int(6 * scale // 50), int(20 * scale // 50)
    if gran1 < 1:
        raise ValueError(f"elastic: 6*scale//50 must be >= 1 (scale={scale}): the noise grid has no spacing")
    return gran1, 40 * scale / 50, gran2, 160 * scale / 50


def blur(noise):
    """The six `scipy.ndimage.convolve(n, ones(3)/3 along one axis, mode='constant')` of the reference, axes
    0,1,2,0,1,2.  Per pass out = f32((l*w + c*w) + r*w) with l, c, r the lower neighbour, the cell and the upper
    neighbour widened to f64 (zero outside the grid) and w = f64(f32(1)/f32(3))."""
    g = np.asarray(noise, np.float32)
    for axis in (0, 1, 2, 0, 1, 2):
        c = g.astype(np.float64)
        lo, hi = np.zeros_like(c), np.zeros_like(c)
        up, down = [slice(None)] * 3, [slice(None)] * 3
        up[axis], down[axis] = slice(1, None), slice(None, -1)
        lo[tuple(up)] = c[tuple(down)]
        hi[tuple(down)] = c[tuple(up)]
        g = ((lo * BLUR_W + c * BLUR_W) + hi * BLUR_W).astype(np.float32)
    return g


def elastic_bb(x, gran):
    """Grid shape of `elastic` for the points x (n, 3): int32(max |x|) // gran + 3 (the cast truncates); a
    sample without points gets 3."""
    if len(x) == 0:
        return np.full(3, 3, np.int64)
    return (np.abs(x).max(0).astype(np.int32) // gran + 3).astype(np.int64)


def _lerp(a, b, f):
    return a * (1 - f) + b * f


def elastic_field(x, noise3, gran, mag):
    """x + g(x) * mag for the three blurred f32 grids noise3, each of shape bb = elastic_bb(x, gran).

    The nodes of axis j are -(bb_j-1)*gran + 2*gran*i (np.linspace(-(b-1)*gran, (b-1)*gran, b)), so with
    u_j = (x_j + (bb_j-1)*gran) / (2*gran), i_j = clip(floor(u_j), 0, bb_j-2), f_j = u_j - i_j each component
    is the trilinear interpolation lerp(a, b, f) = a*(1-f) + b*f along z, then y, then x of the noise widened
    to f64.  All three components are read at the undisplaced x."""
    x = np.asarray(x, np.float64)
    bb = elastic_bb(x, gran)
    for n in noise3:
        if tuple(n.shape) != tuple(bb):
            raise ValueError(f"elastic_field: grid of shape {n.shape}, the points need {tuple(bb)}")
    if len(x) == 0:
        return x.copy()
    idx, frac = [], []
    for j in range(3):
        u = (x[:, j] + (bb[j] - 1) * gran) / (2 * gran)
        i = np.clip(np.floor(u), 0, bb[j] - 2)
        idx.append(i.astype(np.int64))
        frac.append(u - i)
    (i0, i1, i2), (f0, f1, f2) = idx, frac
    out = np.empty_like(x)
    for c in range(3):
        n = noise3[c].astype(np.float64)
        z = [[_lerp(n[i0 + a, i1 + b, i2], n[i0 + a, i1 + b, i2 + 1], f2) for b in (0, 1)] for a in (0, 1)]
        y = [_lerp(z[a][0], z[a][1], f1) for a in (0, 1)]
        out[:, c] = x[:, c] + _lerp(y[0], y[1], f0) * mag
    return out


def elastic(x, raw3, gran, mag):
    """One field of the reference on the raw noise raw3 (three f32 grids of a shape >= bb per axis): the
    [:bb0, :bb1, :bb2] corner is blurred (zeros beyond it) and interpolated."""
    bb = elastic_bb(x, gran)
    for n in raw3:
        if any(s < b for s, b in zip(n.shape, bb)):
            raise ValueError(f"elastic: noise of shape {n.shape} is smaller than the grid {tuple(bb)}")
    return elastic_field(x, [blur(n[:bb[0], :bb[1], :bb[2]]) for n in raw3], gran, mag)


# ---- data-independent grid shapes ----------------------------------------------------------------------------
# cap >= bb.  With A_i >= |a_i| for every point of the sample and t = a . rot,
#   |t_j| <= sum_i A_i |rot_ij| (1 + 2^-52)^3 <= bound1_j + 1
# (the computed bound1 and the three roundings of `transform` are off by a few ulp of a value far below 2^40),
# so int32(max |t_j|) <= int(bound1_j + 1); // gran and + 3 are monotone: bb1_j <= cap1_j.
# A blurred value is an average of noise and zeros: per pass |out| <= max|in| * 3*f32(1/3) * (1 + 2^-24) with
# 3*f32(1/3) = 1 + 3e-8, over six passes <= max|raw| * (1 + 6e-7); the trilinear interpolation is a convex
# combination.  Hence |t1_j| <= |t_j| + mag1 * max|raw_j| * (1 + 6e-7) <= bound1_j + 1 + mag1 * max|raw_j| =
# bound2_j: the + 1 covers the transform's rounding and the 6e-7 excess as long as mag1 * max|raw| < 1e6
# (mag1 = 0.8 * scale, |randn| < 7).  cap2 adds 1 again for the roundings of the field itself.
def elastic_caps(abs_extrema, rot, gran1, mag1=None, gran2=None):
    """(cap1 (3,) int, bound1 (3,) f64) of a sample whose raw points satisfy |a_i| <= abs_extrema_i, under
    t = a . rot: bound1_j = sum_i A_i |rot_ij|, cap1_j = int(bound1_j + 1) // gran1 + 3.  cap2 needs field 1's
    noise as well: `elastic_cap2`."""
    A = np.asarray(abs_extrema, np.float64)
    bound1 = (A[:, None] * np.abs(np.asarray(rot, np.float64))).sum(0)
    cap1 = np.array([int(b + 1) // gran1 + 3 for b in bound1], np.int64)
    return cap1, bound1


def elastic_cap2(bound1, mag1, noise1, gran2):
    """cap2_j = int(bound2_j + 1) // gran2 + 3 with bound2_j = bound1_j + 1 + mag1 * max |raw noise1_j|."""
    bound2 = [bound1[j] + 1 + mag1 * float(np.abs(noise1[j]).max()) for j in range(3)]
    return np.array([int(b + 1) // gran2 + 3 for b in bound2], np.int64)


def elastic_params(scale, seed, idx, caps):
    """The draws of both fields for sample idx: caps = elastic_caps(...) of the sample.  Field 1's three grids
    are randn(*cap1).astype(f32) from RandomState(3000 + seed*997 + idx), then cap2 follows from them and field
    2's grids come from the same stream.  Returns dict(gran1, mag1, gran2, mag2, cap1, cap2, noise1, noise2)."""
    gran1, mag1, gran2, mag2 = elastic_grans(scale)
    cap1, bound1 = caps
    rng = np.random.RandomState(3000 + seed * 997 + idx)
    noise1 = [rng.randn(*cap1).astype(np.float32) for _ in range(3)]
    cap2 = elastic_cap2(bound1, mag1, noise1, gran2)
    noise2 = [rng.randn(*cap2).astype(np.float32) for _ in range(3)]
    return dict(gran1=gran1, mag1=mag1, gran2=gran2, mag2=mag2, cap1=np.asarray(cap1, np.int64), cap2=cap2,
                noise1=noise1, noise2=noise2)


def abs_extrema(points):
    """Per-axis max |raw xyz| (3,) f64 of a scene's float32 points; zeros for an empty scene."""
    points = np.asarray(points, np.float32)
    return np.abs(points).max(0).astype(np.float64) if len(points) else np.zeros(3)


def ball_abs_extrema(scene_extrema, centre, in_radius):
    """The bound of a ball's members: min(scene extrema, |centre| + radius) per axis."""
    return np.minimum(np.asarray(scene_extrema, np.float64), np.abs(np.asarray(centre, np.float64)) + in_radius)


def sample_elastic_params(extrema, rot, scale, seed, idx):
    """elastic_params of a sample with the raw bound `extrema` and the rotation `rot`."""
    gran1, mag1, gran2, _ = elastic_grans(scale)
    return elastic_params(scale, seed, idx, elastic_caps(extrema, rot, gran1, mag1, gran2))


# ---- trainMerge with elastic_deformation ---------------------------------------------------------------------
def merge_elastic_host(samples, params, eparams, full_scale):
    """`trainMerge` over samples [(a, b, c, ids)] (ids: each point's id, or None) with the draws params[i] (of
    `train_params`' shape) and eparams[i] (of `elastic_params`' shape): transform -> field 1 -> field 2 ->
    `_place` -> crop -> `.long()`; the rest as `synthetic.train_merge`.  Returns its dict plus point_ids."""
    locs, feats, labels, scene_labels, point_ids = [], [], [], [], []
    batch_offsets = [0]
    for idx, (a, b, c, ids) in enumerate(samples):
        rot, c1, c2, u1, u2, shift = params[idx]
        e = eparams[idx]
        if len(a):
            t = transform(a, rot, c1, c2)
            t = elastic(t, e["noise1"], e["gran1"], e["mag1"])
            t = elastic(t, e["noise2"], e["gran2"], e["mag2"])
            p, keep = _place(t, u1, u2, full_scale, "train")
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
        point_ids.append((np.arange(len(a)) if ids is None else ids)[keep])
        batch_offsets.append(batch_offsets[-1] + int(keep.sum()))
    return dict(coords=np.concatenate(locs, 0), feats=np.concatenate(feats, 0).astype(np.float32),
                batch_offsets=batch_offsets, labels=np.concatenate(labels, 0),
                scene_labels=np.stack(scene_labels, 0), point_ids=np.concatenate(point_ids, 0).astype(np.int64))


def train_merge_elastic(scenes, scale: float, full_scale: int = 4096, seed: int = 0):
    """`synthetic.train_merge` with `elastic_deformation: True`; the same dict (without point_ids)."""
    params = [train_params(scale, seed, i) for i in range(len(scenes))]
    eparams = [sample_elastic_params(abs_extrema(a), params[i][0], scale, seed, i)
               for i, (a, _, _) in enumerate(scenes)]
    out = merge_elastic_host([(a, b, c, None) for a, b, c in scenes], params, eparams, full_scale)
    del out["point_ids"]
    return out


def train_merge_subcloud_elastic(scenes, entries, scale: float, full_scale: int = 4096, seed: int = 0,
                                 in_radius=2):
    """`subcloud.train_merge_subcloud` with `elastic_deformation: True`: sample b is the ball entries[b] =
    (scene_idx, centre), its grids sized from min(scene extrema, |centre| + in_radius)."""
    start = np.concatenate([[0], np.cumsum([len(a) for a, _, _ in scenes])])
    params = [train_params(scale, seed, i) for i in range(len(entries))]
    samples, eparams = [], []
    for idx, (scene_idx, centre) in enumerate(entries):
        a, b, c = scenes[scene_idx]
        members = np.nonzero(ball_members(a, centre, in_radius))[0]
        samples.append((a[members], b[members], c[members], members + start[scene_idx]))
        ext = ball_abs_extrema(abs_extrema(a), centre, in_radius)
        eparams.append(sample_elastic_params(ext, params[idx][0], scale, seed, idx))
    return merge_elastic_host(samples, params, eparams, full_scale)
