"""The numpy restatement of subcloud-level training samples (wsss3d/subcloud.py; dataset/data.py:69-125, 135-238)
and the argument validation of the device entries (msp_ball_count, msp_merge_ball), without a GPU."""
import ctypes

import numpy as np

from sparseconvnet import _lib
from wsss3d.subcloud import (ball_members, get_anchors, subcloud_anchors, subcloud_counts, subcloud_list,
                             train_merge_subcloud)
from wsss3d.synthetic import make_room, train_merge


def test_get_anchors_order_and_end_points():
    """Extents 4.0 x 2.0 x 0.0 at r = 2: 3 x 2 x 1 anchors, x outermost and z innermost, end points exact."""
    pts = np.array([[-1.5, 0.25, 0.5], [2.5, 2.25, 0.5], [0.0, 1.0, 0.5]], np.float32)
    a = get_anchors(pts, 2)
    assert a.dtype == np.float64 and a.shape == (6, 3)
    want = [[x, y, 0.5] for x in (-1.5, 0.5, 2.5) for y in (0.25, 2.25)]
    assert np.array_equal(a, np.array(want))


def test_get_anchors_extent_of_k_radii_gives_k_plus_one_steps():
    for k in (1, 2, 3):
        pts = np.array([[0, 0, 0], [k * 0.5, 0, 0]], np.float32)
        a = get_anchors(pts, 0.5)
        assert a.shape == (k + 1, 3)
        assert a[0, 0] == 0.0 and a[-1, 0] == k * 0.5
    # just below k radii: k steps
    pts = np.array([[0, 0, 0], [np.nextafter(np.float32(1.5), np.float32(0)), 0, 0]], np.float32)
    assert get_anchors(pts, 0.5).shape == (3, 3)


def test_subcloud_anchors_noise_is_the_seeded_draw():
    a, _, _ = make_room(100, spacing=0.1)
    g = get_anchors(a, 2)
    c = subcloud_anchors(a, 2, seed=3, scene_idx=5)
    noise = np.random.RandomState(3000 + 3 * 997 + 5).normal(scale=0.2, size=g.shape)
    assert c.dtype == np.float64 and np.array_equal(c, g + noise)


def test_membership_against_brute_force_and_boundary():
    rng = np.random.RandomState(0)
    pts = rng.uniform(-3, 3, (500, 3)).astype(np.float32)
    c = np.array([0.25, -0.5, 1.0])
    r = 2.0
    pts[7] = [0.25, 1.5, 1.0]  # distance exactly r (all values exact in binary): kept
    pts[8] = [0.25, np.nextafter(np.float32(1.5), np.float32(2)), 1.0]  # one float32 step further: dropped
    got = ball_members(pts, c, r)
    want = np.zeros(len(pts), bool)
    for i, p in enumerate(pts):
        dx, dy, dz = float(p[0]) - c[0], float(p[1]) - c[1], float(p[2]) - c[2]
        want[i] = ((dx * dx + dy * dy) + dz * dz) <= r * r
    assert np.array_equal(got, want)
    assert got[7] and not got[8]
    assert 0 < got.sum() < len(pts)


def test_min_points_is_greater_or_equal():
    scenes = [make_room(100, spacing=0.1), make_room(101, spacing=0.1)]
    counts = subcloud_counts(scenes, 2, seed=1)
    assert [len(c) for c in counts] == [len(get_anchors(s[0], 2)) for s in scenes]
    k = int(np.argsort(counts[1])[len(counts[1]) // 2])  # an anchor in the middle of scene 1's counts
    n = int(counts[1][k])
    assert n > 0
    kept = subcloud_list(scenes, 2, min_points=n, seed=1)
    assert (1, k) in [(e[0], e[1]) for e in kept]
    assert all(e[3] >= n for e in kept)
    assert [(e[0], e[1]) for e in kept] == sorted((e[0], e[1]) for e in kept)  # scene-then-anchor order
    for s, a, c, cnt in kept:
        assert cnt == counts[s][a] and np.array_equal(c, subcloud_anchors(scenes[s][0], 2, 1, s)[a])
    assert len(kept) == sum(int((c >= n).sum()) for c in counts)
    dropped = subcloud_list(scenes, 2, min_points=n + 1, seed=1)
    assert (1, k) not in [(e[0], e[1]) for e in dropped]


def test_whole_scene_ball_equals_train_merge():
    """A radius that holds the whole scene: train_merge_subcloud is train_merge, field by field."""
    scenes = [make_room(100, spacing=0.1), make_room(101, spacing=0.1)]
    entries = [(i, np.zeros(3)) for i in range(len(scenes))]
    ref = train_merge(scenes, 50, seed=4)
    got = train_merge_subcloud(scenes, entries, 50, seed=4, in_radius=100)
    for k in ("coords", "feats", "labels", "scene_labels"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    assert got["batch_offsets"] == ref["batch_offsets"]
    assert np.array_equal(got["point_ids"], np.arange(sum(len(s[0]) for s in scenes)))


def test_train_merge_subcloud_crops_to_the_ball():
    scenes = [make_room(100, spacing=0.1), make_room(101, spacing=0.1)]
    c = subcloud_anchors(scenes[1][0], 2, 0, 1)[3]
    got = train_merge_subcloud(scenes, [(1, c), (0, np.full(3, 50.0))], 20)
    members = np.nonzero(ball_members(scenes[1][0], c, 2))[0]
    assert 0 < len(members) < len(scenes[1][0])
    assert got["batch_offsets"] == [0, len(members), len(members)]  # the second ball is empty
    assert np.array_equal(got["point_ids"], members + len(scenes[0][0]))
    assert np.array_equal(got["labels"], scenes[1][2][members])
    present = np.unique(scenes[1][2][members])
    want = np.zeros(20, np.float32)
    want[present[present >= 0]] = 1
    assert np.array_equal(got["scene_labels"][0], want) and not got["scene_labels"][1].any()


def test_new_entries_are_prototyped():
    for name in ("msp_ball_count", "msp_merge_ball_workspace_size", "msp_merge_ball"):
        assert name in _lib.PROTOTYPES


def _merge_ball(lib, B=2, mode=0, n_classes=20, ws_bytes=None, scene_of=8, centre=8, r2=4.0):
    p = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = lib.msp_merge_ball_workspace_size(max(B, 1), 5000)
    return lib.msp_merge_ball(None, None, None, None, B, 5000, mode, 4096.0, None, None, None, None, None, None,
                              n_classes, None, None, None, None, 0, None, None, None, ws_bytes, p(scene_of),
                              p(centre), r2, None)


def test_validation_without_gpu():
    """Bad arguments are rejected with -1 and a message before any HIP call (the pointers are never read)."""
    lib = _lib.load()
    assert lib.msp_abi_version() == 10
    assert lib.msp_merge_ball_workspace_size(3, 5000) == lib.msp_merge_workspace_size(3, 5000) > 0
    assert _merge_ball(lib, B=0) == -1 and b"msp_merge_ball" in lib.msp_last_error()
    assert _merge_ball(lib, r2=0.0) == -1 and b"r2" in lib.msp_last_error()
    assert _merge_ball(lib, r2=float("inf")) == -1 and b"r2" in lib.msp_last_error()
    assert _merge_ball(lib, r2=float("nan")) == -1 and b"r2" in lib.msp_last_error()
    assert _merge_ball(lib, ws_bytes=0) == -1 and b"workspace" in lib.msp_last_error()
    assert _merge_ball(lib, scene_of=None) == -1 and b"scene_of" in lib.msp_last_error()
    assert _merge_ball(lib, n_classes=33) == -1 and b"n_classes" in lib.msp_last_error()
    assert _merge_ball(lib, mode=1) == -1 and b"mode" in lib.msp_last_error()
    p = ctypes.c_void_p(8)
    assert lib.msp_ball_count(p, p, 0, 5000, p, p, 4.0, p, None) == -1 and b"msp_ball_count" in lib.msp_last_error()
    assert lib.msp_ball_count(p, p, 2, 5000, p, p, 0.0, p, None) == -1 and b"r2" in lib.msp_last_error()
    assert lib.msp_ball_count(p, p, 2, 5000, p, p, float("nan"), p, None) == -1 and b"r2" in lib.msp_last_error()
    assert lib.msp_ball_count(p, p, 2, 5000, None, p, 4.0, p, None) == -1 and b"null" in lib.msp_last_error()
