"""Elastic distortion in the device batch assembly (wsss3d/merge.py: `elastic=True`, merge_elastic_gpu;
csrc/msp_elastic.hip: msp_merge_elastic) against the numpy restatement (wsss3d/elastic.py) on the same scenes and
draws: coords, feats, labels, offsets and scene labels are compared with array_equal, so there is no tolerance.

Shapes: the assembly block is 1024 points (kMPB), so the batch of `edge_scenes` holds scenes of 1, 1023, 1024 and
1025 points beside a room of several blocks, a scene so small that every |t| < gran1 (bb = 3: cells 0 and 1 only)
and a scene that lies entirely at negative x."""
import functools

import numpy as np
import pytest
import torch

from wsss3d import elastic as E
from wsss3d.merge import DeviceScenes, SubcloudPool, merge_elastic_gpu, train_merge_gpu, train_merge_subcloud_gpu
from wsss3d.synthetic import make_room, train_merge, train_params, transform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sub(room, n, seed):
    idx = np.sort(np.random.RandomState(seed).choice(len(room[0]), n, replace=False))
    return tuple(x[idx] for x in room)


@functools.lru_cache(maxsize=None)
def edge_scenes():
    room = make_room(100, 0.08)
    assert len(room[0]) > 4 * 1024
    tiny = _sub(room, 300, 5)
    tiny = ((tiny[0] * np.float32(0.01)), tiny[1], tiny[2])  # +-3 cm: |t| < 6 at scale 50
    neg = _sub(room, 2000, 6)
    neg = (neg[0] - np.array([4.0, 0, 0], np.float32), neg[1], neg[2])
    assert (neg[0][:, 0] < 0).all()
    return (room, _sub(room, 1, 1), _sub(room, 1023, 2), _sub(room, 1024, 3), _sub(room, 1025, 4), tiny, neg)


@functools.lru_cache(maxsize=None)
def edge_device_scenes():
    return DeviceScenes(list(edge_scenes()))


def _assert_batch_equal(got, ref, ids=False):
    assert got.x.batch_offsets == ref["batch_offsets"]
    assert np.array_equal(got.x.coords.cpu().numpy(), ref["coords"])
    assert np.array_equal(got.x.feature.cpu().numpy(), ref["feats"])
    assert np.array_equal(got.y_orig.cpu().numpy(), ref["labels"])
    assert np.array_equal(got.y.cpu().numpy(), ref["scene_labels"])
    if ids:
        assert np.array_equal(got.point_ids.cpu().numpy(), ref["point_ids"])


def _assert_raw_equal(got, ref):
    coords, feats, labels, ids, off, sl = got
    assert off == ref["batch_offsets"]
    assert np.array_equal(coords.cpu().numpy(), ref["coords"])
    assert np.array_equal(feats.cpu().numpy(), ref["feats"])
    assert np.array_equal(labels.cpu().numpy(), ref["labels"])
    assert np.array_equal(sl.cpu().numpy(), ref["scene_labels"])
    assert np.array_equal(ids.cpu().numpy(), ref["point_ids"])


def _whole(scenes):
    """Whole scenes as merge_elastic_host's samples, each point's id its index into the concatenated scenes."""
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in scenes])])
    return [s + (np.arange(len(s[0])) + start[i],) for i, s in enumerate(scenes)]


def test_block_edges_tiny_mirrored_and_negative_scenes():
    scenes, seed = list(edge_scenes()), 0
    assert [len(s[0]) for s in scenes[1:5]] == [1, 1023, 1024, 1025]
    dets = [np.linalg.det(train_params(50, seed, i)[0]) for i in range(len(scenes))]
    assert min(dets) < 0 < max(dets)  # a mirrored scene (m[0][0] = -1) and an unmirrored one
    gran1 = E.elastic_grans(50)[0]
    rot, c1, c2 = train_params(50, seed, 5)[:3]
    assert E.elastic_bb(transform(scenes[5][0], rot, c1, c2), gran1).tolist() == [3, 3, 3]
    ref = E.train_merge_elastic(scenes, 50, seed=seed)
    plain = train_merge(scenes, 50, seed=seed)
    assert np.abs(ref["coords"] - plain["coords"]).max() >= 1  # the fields move points
    got = train_merge_gpu(edge_device_scenes(), 50, seed=seed, elastic=True)
    _assert_batch_equal(got, ref)


def test_scale_20_bitexact():
    scenes = list(edge_scenes()[:3])
    ref = E.train_merge_elastic(scenes, 20, seed=5)
    got = train_merge_gpu(DeviceScenes(scenes), 20, seed=5, elastic=True)
    _assert_batch_equal(got, ref)


def _lattice_scene():
    """Raw points n/64 (exact in f32): under rot = 64 * I the transform is the integer n.  gran1 = 6*64//50 = 7;
    the lattice spans +-28 = 4 * gran1, so bb1 = 7 with nodes at -42 + 14 i: the points at 0, +-14 and +-28 lie on
    nodes, among them the points at +-|x|max, those at +-7 and +-21 half way between two."""
    k = np.arange(-4, 5) * 7
    n = np.array([[x, y, z] for x in k for y in k for z in k], np.float64)
    rng = np.random.RandomState(3)
    n = np.concatenate([n, rng.randint(-28, 29, (400, 3))])
    a = (n / 64).astype(np.float32)
    assert np.array_equal(a.astype(np.float64) * 64, n)
    return a, rng.rand(len(a), 3).astype(np.float32) * 2 - 1, rng.randint(0, 20, len(a)).astype(np.int64)


def test_points_on_grid_nodes():
    scene = _lattice_scene()
    assert len(scene[0]) > 1024
    rot = np.eye(3) * 64.0
    _, c1, c2, u1, u2, shift = train_params(64, 1, 0)
    params = [(rot, c1, c2, u1, u2, shift)]
    ep = E.sample_elastic_params(E.abs_extrema(scene[0]), rot, 64, 1, 0)
    assert ep["gran1"] == 7
    t = transform(scene[0], rot, c1, c2)
    assert np.array_equal(t, np.round(t)) and E.elastic_bb(t, 7).tolist() == [7, 7, 7]
    ref = E.merge_elastic_host(_whole([scene]), params, [ep], 4096)
    got = merge_elastic_gpu(DeviceScenes([scene]), params, [ep], 4096)
    _assert_raw_equal(got, ref)


def test_cells_beyond_bb_are_never_read():
    """cap > bb: the cells of the drawn grid at or beyond bb hold 1e3 on the device and in the restatement, which
    blurs only the [:bb] corner; one such value leaking into a blur or a read would move points by far."""
    scenes = [edge_scenes()[0], edge_scenes()[4]]
    params = [train_params(50, 2, i) for i in range(2)]
    eparams, grew = [], 0
    for i, (a, _, _) in enumerate(scenes):
        ep = E.sample_elastic_params(E.abs_extrema(a), params[i][0], 50, 2, i)
        t = transform(a, *params[i][:3])
        for f in (1, 2):
            bb = E.elastic_bb(t, ep[f"gran{f}"])
            grew += int((ep[f"cap{f}"] > bb).sum())
            clean = [n.copy() for n in ep[f"noise{f}"]]
            for n in ep[f"noise{f}"]:
                n[bb[0]:], n[:, bb[1]:], n[:, :, bb[2]:] = 1e3, 1e3, 1e3
            assert np.array_equal(E.elastic(t, clean, ep[f"gran{f}"], ep[f"mag{f}"]),
                                  E.elastic(t, ep[f"noise{f}"], ep[f"gran{f}"], ep[f"mag{f}"]))
            t = E.elastic(t, clean, ep[f"gran{f}"], ep[f"mag{f}"])
        eparams.append(ep)
    assert grew >= 6
    ref = E.merge_elastic_host(_whole(scenes), params, eparams, 4096)
    got = merge_elastic_gpu(DeviceScenes(scenes), params, eparams, 4096)
    _assert_raw_equal(got, ref)


def test_crop_with_elastic():
    """Scale 400 into full_scale 1024 (as test_train_merge_gpu_crops): the box crop drops displaced points."""
    scenes = [make_room(7, spacing=0.08)]
    ref = E.train_merge_elastic(scenes, 400, full_scale=1024, seed=1)
    assert 0 < ref["batch_offsets"][-1] < len(scenes[0][0])
    got = train_merge_gpu(DeviceScenes(scenes), 400, full_scale=1024, seed=1, elastic=True)
    _assert_batch_equal(got, ref)


def test_elastic_off_is_the_plain_path_and_calls_repeat():
    scenes = list(edge_scenes()[:3])
    sc = DeviceScenes(scenes)
    plain = train_merge_gpu(sc, 50, seed=3)
    off = train_merge_gpu(sc, 50, seed=3, elastic=False)
    _assert_batch_equal(off, train_merge(scenes, 50, seed=3))
    assert sc._abs_extrema is None  # not computed for callers who never ask
    assert torch.equal(off.x.coords, plain.x.coords) and torch.equal(off.x.feature, plain.x.feature)
    a = train_merge_gpu(sc, 50, seed=3, elastic=True)
    b = train_merge_gpu(sc, 50, seed=3, elastic=True)
    assert np.array_equal(sc.abs_extrema, np.stack([E.abs_extrema(s[0]) for s in scenes]))
    assert a.x.batch_offsets == b.x.batch_offsets
    assert torch.equal(a.x.coords, b.x.coords) and torch.equal(a.x.feature, b.x.feature)
    assert torch.equal(a.y_orig, b.y_orig) and torch.equal(a.y, b.y)
    assert not torch.equal(a.x.coords, plain.x.coords)


@functools.lru_cache(maxsize=None)
def ball_pool():
    return SubcloudPool(edge_device_scenes(), 1.0, min_points=20, seed=0)


def test_two_balls_of_one_scene():
    """Two balls of the room and one of the 1025-point scene in one batch: the displaced coordinates of the two
    are kept apart in the workspace (rows indexed by the sample, not the scene)."""
    p = ball_pool()
    own = [i for i, e in enumerate(p.entries) if e[0] == 0]
    other = [i for i, e in enumerate(p.entries) if e[0] == 4]
    assert len(own) >= 2 and len(other) >= 1
    idx = [own[0], other[0], own[-1]]
    entries = [(p.entries[i][0], p.centre(i)) for i in idx]
    ref = E.train_merge_subcloud_elastic(list(edge_scenes()), entries, 50, seed=3, in_radius=1.0)
    assert np.diff(ref["batch_offsets"]).tolist() == [p.entries[i][2] for i in idx]
    got = train_merge_subcloud_gpu(p, idx, 50, seed=3, elastic=True)
    _assert_batch_equal(got, ref, ids=True)
    plain = train_merge_subcloud_gpu(p, idx, 50, seed=3)
    assert torch.equal(plain.point_ids, got.point_ids) and not torch.equal(plain.x.coords, got.x.coords)


def test_empty_ball_beside_a_normal_one():
    p = ball_pool()
    sc = edge_device_scenes()
    i0 = next(i for i, e in enumerate(p.entries) if e[0] == 0)
    samples = [(0, p.centre(i0)), (0, np.array([50.0, 0.0, 0.0])), (4, np.zeros(3))]
    ref = E.train_merge_subcloud_elastic(list(edge_scenes()), samples, 50, seed=2, in_radius=1.0)
    n0 = p.entries[i0][2]
    assert ref["batch_offsets"][:3] == [0, n0, n0] and ref["batch_offsets"][3] > n0
    params = [train_params(50, 2, b) for b in range(3)]
    ext = sc.abs_extrema
    eparams = [E.sample_elastic_params(E.ball_abs_extrema(ext[s], c, 1.0), params[b][0], 50, 2, b)
               for b, (s, c) in enumerate(samples)]
    got = merge_elastic_gpu(sc, params, eparams, 4096, [s for s, _ in samples], np.stack([c for _, c in samples]),
                            1.0, capacity=ref["batch_offsets"][-1])  # returns only when status == 0
    _assert_raw_equal(got, ref)
    assert not torch.isnan(got[5]).any() and torch.equal(got[5][1], torch.zeros(20, device=got[5].device))


def test_too_small_cap_raises():
    """A grid drawn smaller than the data needs: bb is clamped to cap on the device (every index stays inside the
    sample's grid: i_j <= bb_j - 2 <= cap_j - 2), the status word comes back with the offsets and the call raises."""
    scenes = [edge_scenes()[4]]
    params = [train_params(50, 0, 0)]
    ep = E.sample_elastic_params(E.abs_extrema(scenes[0][0]), params[0][0], 50, 0, 0)
    assert (ep["cap1"] > 3).all()
    ep["cap1"] = np.array([3, 3, 3], np.int64)
    ep["noise1"] = [n[:3, :3, :3].copy() for n in ep["noise1"]]
    sc = DeviceScenes(scenes)
    with pytest.raises(RuntimeError, match="status 1"):
        merge_elastic_gpu(sc, params, [ep], 4096)
    torch.cuda.synchronize()
    ok = train_merge_gpu(sc, 50, seed=0, elastic=True)  # the device is fine afterwards
    assert ok.x.batch_offsets[-1] == 1025
