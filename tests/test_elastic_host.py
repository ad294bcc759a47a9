"""The numpy restatement of the elastic distortion (wsss3d/elastic.py) against the recorded run of the reference's
`elastic` (tests/golden/elastic_field.npz, written by tests/golden/make_elastic_golden.py), the data-independent
grid caps, the unchanged `train_params` draws and msp_merge_elastic's argument validation.  No GPU.

Tolerance of the field: both sides are fp64 and differ in evaluation order only (scipy's interpolator normalises
the coordinate against the node values, the restatement against gran), a few ulp of coordinates of some hundred
voxels, ~1e-13; 1e-9 voxels leaves four orders of margin and is 1e3 below the fixture's guaranteed 1e-6 clearance
from an integer, so the truncated coordinates are compared on every point."""
import os

import numpy as np
import pytest

from sparseconvnet import _lib
from wsss3d import elastic as E
from wsss3d.synthetic import make_room, train_merge, train_params, transform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "elastic_field.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("scale", [50, 20])
def test_fields_match_the_reference(golden, scale):
    g = golden
    assert E.elastic_grans(scale) == (int(g[f"gran1_{scale}"]), float(g[f"mag1_{scale}"]),
                                      int(g[f"gran2_{scale}"]), float(g[f"mag2_{scale}"]))
    x = g[f"x_{scale}"]
    assert len(x) == 2000
    for f in (1, 2):
        gran, mag = int(g[f"gran{f}_{scale}"]), float(g[f"mag{f}_{scale}"])
        want = g[f"y{f}_{scale}"]
        assert np.array_equal(E.elastic_bb(x, gran), g[f"bb{f}_{scale}"])
        got = E.elastic(x, list(g[f"raw{f}_{scale}"]), gran, mag)
        err = np.abs(got - want).max()
        print(f"scale {scale} field {f}: max |ours - reference| = {err:.3e}")
        assert err <= 1e-9
        assert np.abs(want - np.round(want)).min() > 1e-6
        assert np.array_equal(got.astype(np.int64), want.astype(np.int64))
        x = want  # the reference's own input of field 2


@pytest.mark.parametrize("scale", [50, 20])
def test_blur_matches_the_reference(golden, scale):
    """Within one f32 ulp of the grids the reference handed to its interpolator; reports whether bit-equal."""
    for f in (1, 2):
        want = golden[f"blur{f}_{scale}"]
        got = np.stack([E.blur(r) for r in golden[f"raw{f}_{scale}"]])
        assert got.dtype == np.float32 and got.shape == want.shape
        print(f"scale {scale} field {f}: blur bit-equal to scipy: {np.array_equal(got, want)}")
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()


def test_blur_pads_with_zeros():
    one = np.zeros((3, 4, 5), np.float32)
    one[0, 0, 0] = 1
    b = E.blur(one)
    assert b[0, 0, 0] > 0 and b[2, 2, 2] > 0 and (b[:, 3:, :] == 0).all() and (b[:, :, 3:] == 0).all()
    # a corner cell loses mass to the padding: per axis 2/3 after the first pass, (2/3 + 1) / 3 after the second
    assert abs(float(E.blur(np.ones((3, 3, 3), np.float32))[0, 0, 0]) - (5 / 9) ** 3) < 1e-6


def test_bb_edges():
    gran = 6
    x = np.array([[2.0 * gran, 1.0, -1.0], [-3.0, 2.0, 0.5]])
    assert E.elastic_bb(x, gran).tolist() == [5, 3, 3]  # |x|max exactly 2*gran
    assert E.elastic_bb(np.array([[5.999, -5.5, 0.0]]), gran).tolist() == [3, 3, 3]  # all inside gran
    assert E.elastic_bb(np.array([[-6.0, 11.999, 12.0]]), gran).tolist() == [4, 4, 5]
    assert E.elastic_bb(np.zeros((0, 3)), gran).tolist() == [3, 3, 3]
    noise = [np.random.RandomState(c).randn(5, 3, 3).astype(np.float32) for c in range(3)]
    assert np.isfinite(E.elastic_field(x, noise, gran, 2.0)).all()


def test_field_on_grid_nodes_is_the_node_value():
    gran, mag = 4, 3.0
    bb = np.array([4, 3, 3])
    noise = [np.random.RandomState(10 + c).randn(*bb).astype(np.float32) for c in range(3)]
    nodes = np.array([[-(bb[0] - 1) * gran + 2 * gran * i, -(bb[1] - 1) * gran + 2 * gran * j,
                       -(bb[2] - 1) * gran + 2 * gran * k] for i in range(4) for j in range(3) for k in range(3)],
                     np.float64)
    # the nodes that keep bb at (4, 3, 3), and one point off the nodes that pins it there
    pts = np.concatenate([nodes[(np.abs(nodes) <= [7, 3, 3]).all(1)], [[7.5, 3.5, -3.5]]])
    assert len(pts) == 3
    assert E.elastic_bb(pts, gran).tolist() == bb.tolist()
    y = E.elastic_field(pts, noise, gran, mag)
    for p, q in zip(pts[:-1], y[:-1]):
        i, j, k = ((p + (bb - 1) * gran) / (2 * gran)).astype(int)
        assert np.array_equal(q, p + np.array([n[i, j, k] for n in noise], np.float64) * mag)


def test_gran_must_be_positive():
    with pytest.raises(ValueError, match="6\\*scale//50"):
        E.elastic_grans(8)
    assert E.elastic_grans(9)[0] == 1


def test_caps_cover_bb_over_random_rotations():
    """cap >= bb for both fields over 200 random scenes and rotations, scales from 9 to 400."""
    rng = np.random.RandomState(5)
    slack = []
    for k in range(200):
        scale = [9, 20, 50, 400][k % 4]
        a = ((rng.rand(300, 3) - 0.5) * rng.uniform(0.5, 6, 3)).astype(np.float32)
        rot, c1, c2 = train_params(scale, k, 0)[:3]
        ep = E.sample_elastic_params(E.abs_extrema(a), rot, scale, k, 0)
        t = transform(a, rot, c1, c2)
        bb1 = E.elastic_bb(t, ep["gran1"])
        assert (ep["cap1"] >= bb1).all(), (k, ep["cap1"], bb1)
        t1 = E.elastic(t, ep["noise1"], ep["gran1"], ep["mag1"])
        bb2 = E.elastic_bb(t1, ep["gran2"])
        assert (ep["cap2"] >= bb2).all(), (k, ep["cap2"], bb2)
        slack.append((ep["cap1"] / bb1).max())
    assert max(slack) < 4  # the bound is not vacuous


def test_cap_shaped_draw_equals_its_corner():
    rng = np.random.RandomState(2)
    x = (rng.rand(500, 3) - 0.5) * [200, 150, 100]
    gran, mag = 6, 40.0
    bb = E.elastic_bb(x, gran)
    big = [rng.randn(*(bb + [4, 1, 7])).astype(np.float32) for _ in range(3)]
    corner = [n[:bb[0], :bb[1], :bb[2]].copy() for n in big]
    assert np.array_equal(E.elastic(x, big, gran, mag), E.elastic(x, corner, gran, mag))
    poisoned = [n.copy() for n in big]
    for n in poisoned:
        n[bb[0]:], n[:, bb[1]:], n[:, :, bb[2]:] = 1e3, 1e3, 1e3
    assert np.array_equal(E.elastic(x, poisoned, gran, mag), E.elastic(x, corner, gran, mag))
    with pytest.raises(ValueError, match="smaller"):
        E.elastic(x, [n[:bb[0] - 1] for n in big], gran, mag)


def test_train_merge_elastic_moves_points_and_keeps_the_rest():
    scenes = [make_room(40 + i, spacing=0.08) for i in range(2)]
    plain = train_merge(scenes, 50, seed=4)
    el = E.train_merge_elastic(scenes, 50, seed=4)
    assert el["batch_offsets"] == plain["batch_offsets"]  # nothing cropped at 4096
    assert np.array_equal(el["feats"], plain["feats"]) and np.array_equal(el["labels"], plain["labels"])
    assert np.array_equal(el["scene_labels"], plain["scene_labels"])
    d = np.abs(el["coords"][:, :3] - plain["coords"][:, :3]).max()
    assert 1 <= d < 4096
    assert np.array_equal(el["coords"][:, 3], plain["coords"][:, 3])


def test_subcloud_elastic_of_a_whole_scene_ball_sizes_grids_from_the_ball():
    scenes = [make_room(41, spacing=0.08)]
    centre = np.array([0.3, -0.2, 0.1])
    out = E.train_merge_subcloud_elastic(scenes, [(0, centre), (0, centre + 40.0)], 50, seed=1, in_radius=1.0)
    n = int(((scenes[0][0].astype(np.float64) - centre) ** 2).sum(1).__le__(1.0).sum())
    assert out["batch_offsets"] == [0, n, n] and n > 100
    ext = E.ball_abs_extrema(E.abs_extrema(scenes[0][0]), centre, 1.0)
    assert (ext <= np.abs(centre) + 1.0).all() and (ext <= E.abs_extrema(scenes[0][0])).all()


def test_train_params_draws_are_unchanged():
    rot, c1, c2, u1, u2, shift = train_params(50, 3, 2)
    assert rot.ravel().tolist() == [-19.421053003428074, 45.25357567809761, 7.130456633176985, -35.913085610744965,
                                    -18.978025470480237, 5.043526087789147, -0.012152122319153105,
                                    -2.326882399185886, 49.40249294391216]
    assert c1.tolist() == [0.0, 0.0, 0.0] and c2.tolist() == [0.0, 0.0, 0.0]
    assert u1.tolist() == [0.9697632476215988, 0.0697844017882614, 0.5001714858017858]
    assert u2.tolist() == [0.6143871711975436, 0.24289073098304403, 0.20594116960458841]
    assert shift.dtype == np.float32
    assert shift.tolist() == [np.float32(x) for x in (0.009002581238746643, 0.026525354012846947,
                                                      -0.20858044922351837)]


def _elastic_args(**over):
    """msp_merge_elastic's arguments with dummy non-null pointers (never dereferenced: the call is rejected)."""
    p = 64
    a = dict(xyz=p, rgb=p, labels=p, scene_start=p, B=2, max_scene_points=100, mode=0, full_scale=4096.0, rot=p,
             c1=p, c2=p, u1=p, u2=p, shift=p, n_classes=20, coords=p, feats=p, labels_out=p, point_ids=p,
             point_id_base=0, batch_offsets=p, scene_labels=p, ws=p, ws_bytes=0, scene_of=None, centre=None, r2=0.0,
             noise1=p, noise2=p, cap1=p, cap2=p, cell_off1=p, cell_off2=p, cap_cells_total=1000, gran1=6, mag1=40.0,
             gran2=20, mag2=160.0, status=p, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def test_validation_without_gpu():
    lib = _lib.load()
    assert lib.msp_abi_version() == 10
    need = _lib.query("msp_merge_elastic_workspace_size", 2, _lib.I64(100), _lib.I64(1000))
    base = _lib.query("msp_merge_workspace_size", 2, _lib.I64(100))
    # two ping-pong grids of 3 * 1000 f32 and 3 f64 per slot of 2 samples x 1 block x 1024 points on top
    assert need >= base + 2 * 3 * 1000 * 4 + 2 * 1024 * 3 * 8
    for over, msg in ((dict(gran1=0), b"gran"), (dict(gran2=-3), b"gran"), (dict(noise1=None), b"null"),
                      (dict(noise2=None), b"null"), (dict(cap1=None), b"null"), (dict(status=None), b"status"),
                      (dict(mag1=float("inf")), b"finite"), (dict(mag2=float("nan")), b"finite"),
                      (dict(B=0), b"bad arguments"), (dict(mode=1), b"mode"),
                      (dict(scene_of=64), b"scene_of"), (dict(ws_bytes=need - 1), b"workspace too small")):
        rc = lib.msp_merge_elastic(*_elastic_args(**over))
        assert rc == -1 and msg in lib.msp_last_error(), (over, lib.msp_last_error())
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call("msp_merge_elastic", *_elastic_args())
