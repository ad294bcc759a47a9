"""Subcloud-level training batches assembled on the device (wsss3d/merge.py: SubcloudPool,
train_merge_subcloud_gpu; msp_ball_count, msp_merge_ball) against the numpy restatement (wsss3d/subcloud.py;
dataset/data.py:69-125, 135-238) on the same scenes and draws: counts, lists, integer outputs and colours are
compared with array_equal, so there is no tolerance.

Scenes: three procedural rooms (39,105 / 44,851 / 23,945 points) and two index-sorted subsamples of the first
with 1025 and 1023 points: the assembly block is 1024 points, so one full block plus one point, and one short of
a block.  At r = 2 the rooms give 18 / 18 / 12 anchors; at r = 0.5 they give 660 / 594 / 480, of which some
hundred are empty and some hundred hold >= 200 points: kept, dropped and empty balls, and more anchors than one
256-centre LDS chunk of the count kernel.  The tests assert those conditions on the restatement's counts before
they compare, so a drifting generator cannot hollow them out."""
import functools

import numpy as np
import pytest
import torch

from sparseconvnet import _lib
from sparseconvnet._lib import call, ptr
from wsss3d import EasyDict, LOSS_REGISTRY, MODEL_REGISTRY
from wsss3d.merge import DeviceScenes, SubcloudPool, train_merge_gpu, train_merge_subcloud_gpu
from wsss3d.subcloud import subcloud_counts, subcloud_list, train_merge_subcloud
from wsss3d.synthetic import make_room, train_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS_CHUNK = 256  # centres per staged chunk in ball_count_kernel (csrc/msp_merge.hip: kBC)


@functools.lru_cache(maxsize=None)
def scenes():
    rooms = [make_room(100, 0.05), make_room(101, 0.05), make_room(102, 0.06)]
    assert [len(r[0]) for r in rooms] == [39105, 44851, 23945]
    out = list(rooms)
    for n, s in ((1025, 7), (1023, 8)):
        idx = np.sort(np.random.RandomState(s).choice(len(rooms[0][0]), n, replace=False))
        out.append(tuple(x[idx] for x in rooms[0]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def device_scenes():
    return DeviceScenes(list(scenes()))


@functools.lru_cache(maxsize=None)
def ref_counts(r):
    return subcloud_counts(list(scenes()), r, seed=0)


@functools.lru_cache(maxsize=None)
def pool(r, min_points):
    return SubcloudPool(device_scenes(), r, min_points=min_points, seed=0)


def _check_premises(r):
    c = ref_counts(r)
    if r == 2:
        assert [len(x) for x in c[:3]] == [18, 18, 12]
    else:
        assert all(len(x) > LDS_CHUNK for x in c[:3])  # more anchors than one LDS chunk
        for x in c[:3]:
            assert (x == 0).sum() > 0 and (x >= 200).sum() > 0 and ((x > 0) & (x < 200)).sum() > 0


@pytest.mark.parametrize("r", [2, 0.5])
def test_counts_equal_the_restatement(r):
    _check_premises(r)
    got = pool(r, 200).counts
    ref = ref_counts(r)
    assert len(got) == len(ref) == 5
    for g, w in zip(got, ref):
        assert g.dtype == np.int64 and np.array_equal(g, w)


@pytest.mark.parametrize("r", [2, 0.5])
def test_list_equals_the_restatement(r):
    """min_points equal to one anchor's own count: that anchor is kept (>=)."""
    _check_premises(r)
    c = ref_counts(r)[1]
    k = int(np.argsort(c)[2 * len(c) // 3])
    n = int(c[k])
    assert n > 0 and (c < n).any()
    ref = subcloud_list(list(scenes()), r, min_points=n, seed=0)
    p = SubcloudPool(device_scenes(), r, min_points=n, seed=0)
    assert len(p) == len(ref) and (1, k, n) in p.entries
    assert p.entries == [(s, a, cnt) for s, a, _, cnt in ref]
    centres = p.centres.cpu().numpy()
    for i, (s, a, centre, _) in enumerate(ref):
        assert np.array_equal(p.centre(i), centre)
        assert np.array_equal(centres[p.anchor_start[s] + a], centre)


def test_min_points_below_one_is_rejected():
    with pytest.raises(ValueError, match="min_points"):
        SubcloudPool(device_scenes(), 2, min_points=0)


def _pick(p, per_scene=(3, 2, 2, 1, 1), seed=0):
    """Indices into p.entries: per_scene[s] balls of scene s, shuffled."""
    rng = np.random.RandomState(seed)
    out = []
    for s, n in enumerate(per_scene):
        own = [i for i, e in enumerate(p.entries) if e[0] == s]
        assert len(own) >= n, (s, len(own))
        out += list(rng.choice(own, n, replace=False))
    rng.shuffle(out)
    return [int(i) for i in out]


def _assert_batch_equal(got, ref):
    assert got.x.batch_offsets == ref["batch_offsets"]
    assert np.array_equal(got.x.coords.cpu().numpy(), ref["coords"])
    assert np.array_equal(got.x.feature.cpu().numpy(), ref["feats"])
    assert np.array_equal(got.y_orig.cpu().numpy(), ref["labels"])
    assert np.array_equal(got.y.cpu().numpy(), ref["scene_labels"])
    assert np.array_equal(got.point_ids.cpu().numpy(), ref["point_ids"])


@pytest.mark.parametrize("r,min_points,scale", [(2, 200, 50), (0.5, 20, 20)])
def test_batch_bitexact(r, min_points, scale):
    """Nine balls in shuffled order, three of them from one scene, one each from the 1025- and the 1023-point
    scene."""
    p = pool(r, min_points)
    idx = _pick(p)
    assert len(idx) == 9 and [p.entries[i][0] for i in idx] != sorted(p.entries[i][0] for i in idx)
    entries = [(p.entries[i][0], p.centre(i)) for i in idx]
    ref = train_merge_subcloud(list(scenes()), entries, scale, seed=3, in_radius=r)
    got = train_merge_subcloud_gpu(p, idx, scale, seed=3)
    assert np.diff(ref["batch_offsets"]).tolist() == [p.entries[i][2] for i in idx]  # nothing cropped at 4096
    _assert_batch_equal(got, ref)


def test_batch_crops_after_the_ball():
    """Scale 400 into full_scale 1024 (as test_train_merge_gpu_crops): the box crop drops rows of the ball."""
    p = pool(2, 200)
    idx = _pick(p, per_scene=(2, 1, 1, 1, 0), seed=1)
    entries = [(p.entries[i][0], p.centre(i)) for i in idx]
    ref = train_merge_subcloud(list(scenes()), entries, 400, full_scale=1024, seed=1, in_radius=2)
    got = train_merge_subcloud_gpu(p, idx, 400, full_scale=1024, seed=1)
    kept, members = np.diff(ref["batch_offsets"]), np.array([p.entries[i][2] for i in idx])
    assert (kept <= members).all() and (kept < members).any() and kept.sum() > 0
    _assert_batch_equal(got, ref)


def test_whole_scene_ball_equals_train_merge_gpu():
    """r = 100: one anchor per scene, every point a member; the ball path reproduces the scene path, which is
    itself pinned by tests/test_gpu_merge.py."""
    sc = DeviceScenes(list(scenes()[1:4]))
    p = SubcloudPool(sc, 100, min_points=1, seed=0)
    assert p.entries == [(i, 0, len(s[0])) for i, s in enumerate(scenes()[1:4])]
    ref = train_merge_gpu(sc, 50, seed=2)
    got = train_merge_subcloud_gpu(p, range(3), 50, seed=2)
    assert got.x.batch_offsets == ref.x.batch_offsets
    assert torch.equal(got.x.coords, ref.x.coords) and torch.equal(got.x.feature, ref.x.feature)
    assert torch.equal(got.y_orig, ref.y_orig) and torch.equal(got.y, ref.y)
    assert torch.equal(got.point_ids, torch.arange(sc.start[-1], device=got.point_ids.device))


def _merge_ball_raw(sc, samples, r2, params, full_scale=4096):
    """msp_merge_ball called directly: samples = [(scene, centre)], params = the per-sample draws.  Outputs are
    sized by the scenes' points and poisoned, so a stray or NaN write would show."""
    B = len(samples)
    f64 = dict(dtype=torch.float64, device=DEV)
    rot = torch.tensor(np.stack([q[0] for q in params]).reshape(B, 9), **f64)
    c1, c2, u1, u2 = (torch.tensor(np.stack([q[k] for q in params]), **f64) for k in (1, 2, 3, 4))
    shift = torch.tensor(np.stack([q[5] for q in params]), dtype=torch.float32, device=DEV)
    scene_of = torch.tensor([s for s, _ in samples], dtype=torch.int32, device=DEV)
    centre = torch.tensor(np.stack([c for _, c in samples]), **f64)
    cap = sum(sc.start[s + 1] - sc.start[s] for s, _ in samples)
    coords = torch.full((cap, 4), -7, dtype=torch.int64, device=DEV)
    feats = torch.full((cap, 3), -7.0, dtype=torch.float32, device=DEV)
    labels = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    ids = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    offsets = torch.full((B + 1,), -7, dtype=torch.int64, device=DEV)
    scene_labels = torch.full((B, 20), -7.0, dtype=torch.float32, device=DEV)
    wsb = int(_lib.query("msp_merge_ball_workspace_size", B, _lib.I64(sc.max_points)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    call("msp_merge_ball", ptr(sc.xyz), ptr(sc.rgb), ptr(sc.labels), ptr(sc.start_dev), B, sc.max_points, 0,
         float(full_scale), ptr(rot), ptr(c1), ptr(c2), ptr(u1), ptr(u2), ptr(shift), 20, ptr(coords), ptr(feats),
         ptr(labels), ptr(ids), 0, ptr(offsets), ptr(scene_labels), ptr(ws), wsb, ptr(scene_of), ptr(centre),
         float(r2), _lib.stream(torch.device(DEV)))
    return coords, feats, labels, ids, offsets.tolist(), scene_labels


def test_empty_ball_is_harmless():
    """A sample whose centre lies 50 m away, between two ordinary samples: zero rows, equal neighbouring
    offsets, an all-zero label row, nothing written past the kept rows, the other samples unchanged."""
    sc = device_scenes()
    p = pool(2, 200)
    i0, i1 = _pick(p, per_scene=(1, 0, 0, 1, 0), seed=2)
    s0, s1 = (p.entries[i0][0], p.centre(i0)), (p.entries[i1][0], p.centre(i1))
    far = (1, np.array([50.0, 0.0, 0.0]))
    q = [train_params(20, 5, b) for b in range(3)]
    co3, fe3, la3, id3, off3, sl3 = _merge_ball_raw(sc, [s0, far, s1], 4.0, q)
    co2, fe2, la2, id2, off2, sl2 = _merge_ball_raw(sc, [s0, s1], 4.0, [q[0], q[2]])
    n0, n1 = p.entries[i0][2], p.entries[i1][2]
    assert off3 == [0, n0, n0, n0 + n1] and off2 == [0, n0, n0 + n1]
    n = n0 + n1
    assert torch.equal(sl3[1], torch.zeros(20, device=DEV))
    assert torch.equal(sl3[[0, 2]], sl2) and not torch.isnan(sl3).any()
    assert torch.equal(co3[:n, :3], co2[:n, :3])
    assert torch.equal(co3[:n, 3], torch.tensor([0] * n0 + [2] * n1, device=DEV))
    assert torch.equal(fe3[:n], fe2[:n]) and torch.equal(la3[:n], la2[:n]) and torch.equal(id3[:n], id2[:n])
    for t in (co3, fe3, la3, id3):  # the rows past the kept ones still hold the poison
        assert (t[n:] == -7).all()


def test_one_training_step_on_a_ball_batch():
    torch.manual_seed(0)
    p = pool(2, 200)
    idx = _pick(p, per_scene=(2, 1, 1, 0, 0), seed=3)
    batch = train_merge_subcloud_gpu(p, idx, 20, seed=1)
    assert batch.y.shape == (4, 20)
    off = batch.x.batch_offsets
    for b in range(4):
        lab = batch.y_orig[off[b]:off[b + 1]]
        want = torch.zeros(20, device=DEV)
        want[torch.unique(lab[lab >= 0])] = 1
        assert torch.equal(batch.y[b], want)
    pc = EasyDict(name="SparseConvFCNetDirectUpPool", m=16, dimension=3, full_scale=4096, block_reps=1,
                  residual_blocks=False)
    model = MODEL_REGISTRY.get("MultiLabel")[0](pc).to(DEV)
    logits, _ = model((batch.x, None), istrain=True)
    assert logits.shape == (4, 20) and torch.isfinite(logits).all()
    loss = LOSS_REGISTRY.get("Classification")[0](logits, batch.y)
    loss.backward()
    assert torch.isfinite(loss)
    for name, w in model.named_parameters():
        assert w.grad is not None and torch.isfinite(w.grad).all(), name
