"""The metadata kernels (csrc/msp_meta.hip, the scans of msp_core.hip) entry by entry against the plain numpy
restatements of tests/metadata_ref.py, at grid faces and corners, tile and scan-block edges.

Every comparison is integer-exact; the one numeric check (InputLayer averaging under heavy duplication) uses the
bound of a sequential fp32 sum.  The clouds are built here with fixed seeds as plain numpy (no device), so
tests/test_metadata_ref.py can assert that they hold the edges the tests below rely on.
"""
import functools

import numpy as np
import pytest
import torch

import metadata_ref as R
import sparseconvnet as scn
from sparseconvnet import _lib, metadata
from sparseconvnet._lib import I64, call, ptr, query
from wsss3d.synthetic import random_cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------- clouds (numpy, fixed seeds; never modified)
@functools.lru_cache(maxsize=None)
def full16_cloud():
    """Every site of a 16^3 grid in batch 0 and in batch 1, each point twice, shuffled (16384 points)."""
    g = np.arange(16)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    c = np.concatenate([np.concatenate([xyz, np.full((4096, 1), b)], 1) for b in (0, 1)]).astype(np.int64)
    c = np.concatenate([c, c])
    return c[np.random.default_rng(16).permutation(len(c))]


def _corners4096_points():
    rng = np.random.default_rng(4096)
    S = 4096
    parts = []

    def add(xyz, b):
        xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
        parts.append(np.concatenate([xyz, np.full((len(xyz), 1), b, np.int64)], 1))

    corners = np.array([[x, y, z] for x in (0, S - 1) for y in (0, S - 1) for z in (0, S - 1)])
    add(corners, 0)
    add(corners, 3)
    g = np.arange(16)
    blk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    low = blk[rng.random(len(blk)) < 0.5]                     # 16^3 block at the origin, half occupied
    top = blk[rng.random(len(blk)) < 0.5] + (S - 16)          # and at (4080..4095)^3
    add(low, 0)
    add(top, 0)
    # what a neighbour past a face of batch 0 would alias if its key were formed: the same site modulo the grid
    # in the adjacent batch (the key space is contiguous across batches)
    for ax in range(3):
        on_face = top[top[:, ax] == S - 1][:60].copy()
        on_face[:, ax] = 0
        add(on_face, 1)
        on_face = low[low[:, ax] == 0][:60].copy()
        on_face[:, ax] = S - 1
        add(on_face, 1)
    # a slab straddling x = 2047 / 2048 (the top Morton bit of x)
    slab = np.stack([rng.integers(2046, 2050, 500), rng.integers(2040, 2056, 500), rng.integers(2040, 2056, 500)], 1)
    add(slab, 1)
    # points on each face
    for ax in range(3):
        for side in (0, S - 1):
            p = rng.integers(0, S, (50, 3))
            p[:, ax] = side
            add(p, 3 if ax % 2 else 0)
    pts = np.concatenate(parts)
    pts = np.concatenate([pts, pts[rng.integers(0, len(pts), len(pts) // 8)]])   # duplicates
    return pts[rng.permutation(len(pts))]


@functools.lru_cache(maxsize=None)
def corners4096_cloud(sorted_batches=True):
    """Size 4096, batch ids {0, 1, 3}: the 8 corners, half-occupied 16^3 blocks at the origin and at
    (4080..4095)^3, a slab across x = 2047/2048, points on every face; batch column sorted or shuffled."""
    pts = _corners4096_points()
    if sorted_batches:
        pts = pts[np.argsort(pts[:, 3], kind="stable")]
    return pts


@functools.lru_cache(maxsize=None)
def sparse_cloud(V):
    """random_cloud at size 64 trimmed to exactly V voxels (a random subset of its voxels, every point of them)."""
    coords, _ = random_cloud(1500, 64, n_batch=2, seed=V, dense_frac=0.3)
    _, inv = np.unique(R.raster_key(coords, 64), return_inverse=True)
    inv = inv.reshape(-1)
    assert inv.max() + 1 >= V
    keep = np.random.default_rng(V).permutation(inv.max() + 1)[:V]
    return coords[np.isin(inv, keep)]


@functools.lru_cache(maxsize=None)
def one_cloud():
    return np.array([[4095, 0, 4095, 0]], np.int64)


@functools.lru_cache(maxsize=None)
def single_child_cloud():
    """Size 64: one site in each of 700 distinct 4^3 blocks, so every coarse site of stride 2 and of stride 4 has
    exactly one child."""
    rng = np.random.default_rng(7)
    blocks = np.unique(rng.integers(0, 16, (900, 3)), axis=0)[:700]
    xyz = blocks * 4 + rng.integers(0, 4, blocks.shape)
    return np.concatenate([xyz, rng.integers(0, 2, (len(xyz), 1))], 1).astype(np.int64)


CLOUDS = {
    "full16": (full16_cloud, 16),
    "corners4096": (corners4096_cloud, 4096),
    "corners4096_shuffled": (functools.partial(corners4096_cloud, False), 4096),
    "sparse512": (functools.partial(sparse_cloud, 512), 64),
    "sparse513": (functools.partial(sparse_cloud, 513), 64),
    "one": (one_cloud, 4096),
    "single_child": (single_child_cloud, 64),
}


# ---------------------------------------------------------------- shared builds and references
def _np(t):
    return t.detach().cpu().numpy()


def _u64(t):
    return _np(t).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _built(name):
    """Device level 0 of a cloud and its reference, built once and shared (read-only) by the tests."""
    fn, size = CLOUDS[name]
    coords = fn()
    log2 = int(np.log2(size))
    assert 1 << log2 == size
    meta = metadata.Metadata(DEV)
    lvl = meta.build_input(torch.from_numpy(coords), size)
    ref = R.voxelise(coords, log2)
    ref_coords = R.decode_key(ref["keys"], log2)
    dev_coords = _np(meta.locations(size))
    return dict(coords=coords, size=size, log2=log2, meta=meta, lvl=lvl, ref=ref, ref_coords=ref_coords,
                dev_coords=dev_coords)


@functools.lru_cache(maxsize=None)
def _ref_subm(name, f):
    """The reference neighbour map in the DEVICE's row order (rows matched through their coordinates)."""
    b = _built(name)
    m = R.subm_map(b["ref_coords"], b["size"], f)
    to_ref = R.row_map(b["dev_coords"], b["ref_coords"], b["size"])
    to_dev = np.empty_like(to_ref)
    to_dev[to_ref] = np.arange(len(to_ref))
    return np.where(m >= 0, to_dev[np.maximum(m, 0)], -1).astype(np.int32)[:, to_ref]


# ---------------------------------------------------------------- 1. keys, segments, decode
@pytest.mark.parametrize("name", ["full16", "corners4096", "corners4096_shuffled", "sparse512", "sparse513", "one"])
def test_keys_segments_decode(name):
    """msp_point_keys, msp_sort_pairs, msp_segment (shift 0, with p2v) and msp_decode_keys through
    Metadata.build_input.  Scan path: msp_segment's one-block scan of ceil(n/2048) block sums, a single pass
    (at most 9 blocks here)."""
    b = _built(name)
    lvl, meta, ref, n = b["lvl"], b["meta"], b["ref"], len(b["coords"])
    V = len(ref["keys"])
    assert lvl.n == V
    keys = _u64(lvl.keys)[:V]
    assert (keys[1:] > keys[:-1]).all(), "level keys strictly ascending"
    assert np.array_equal(keys, ref["keys"])
    assert np.array_equal(b["dev_coords"], b["ref_coords"]), "decoded locations"
    inp = meta.input
    assert np.array_equal(_np(inp.p2v).astype(np.int64), ref["p2v"])
    vstart = _np(inp.vstart).astype(np.int64)
    assert np.array_equal(vstart, ref["vstart"])
    perm = _np(inp.perm).astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(n)), "perm is a permutation of the points"
    assert np.array_equal(R.canonical_lists(perm, vstart), ref["order"]), "per-voxel point sets"
    bcol = b["coords"][:, 3]
    monotonic = bool((np.diff(bcol) >= 0).all())
    assert inp.batch_monotonic == monotonic
    assert inp.batch_size == bcol.max() + 1
    if monotonic:
        assert inp.scene_starts == np.searchsorted(bcol, np.arange(bcol.max() + 2), side="left").tolist()
    else:
        assert inp.scene_starts is None


def test_scene_starts_skip_an_absent_batch_id():
    """corners4096 has batch ids {0, 1, 3}: the sorted copy's scene starts are the lower bounds of ids 0..4, the
    absent id 2 giving two equal consecutive starts; the shuffled copy is not monotonic."""
    b = _built("corners4096")
    bcol = b["coords"][:, 3]
    assert sorted(set(bcol.tolist())) == [0, 1, 3]
    st = b["meta"].input.scene_starts
    assert len(st) == 5 and st[0] == 0 and st[4] == len(bcol)
    assert st == [int((bcol < i).sum()) for i in range(5)]
    assert st[2] == st[3] and st[1] < st[2] < st[4]
    assert _built("corners4096_shuffled")["meta"].input.batch_monotonic is False


@pytest.mark.parametrize("size", [64, 60])
def test_point_keys_direct_bad_rows_and_stats(size):
    """msp_point_keys called directly with row_stride = 6 and bad rows (x = -1, x = size, batch = -1, ...) mixed
    into good ones, some at the 256-thread block edges: stats == [n_bad, largest GOOD batch id, descents of the
    batch column], bad rows get the all-ones key.  size 60 in a 64 grid: 60..63 fit the key's bits and are bad."""
    rng = np.random.default_rng(size)
    n, log2 = 1000, 6
    rows = np.empty((n, 6), np.int64)
    rows[:, :3] = rng.integers(0, size, (n, 3))
    rows[:, 3] = rng.integers(0, 6, n)
    rows[:, 4] = -7
    rows[:, 5] = 1 << 40
    rows[[3, 500], 0] = size - 1                       # on the face: good
    rows[[4, 501], 2] = 0
    bad = {0: (0, -1), 255: (0, size), 256: (3, -1), 511: (1, size), 512: (2, -1), 700: (2, size + 5), 999: (1, -3)}
    for i, (col, v) in bad.items():
        rows[i, col] = v
    rows[640, 0], rows[640, 3] = size, 9                # a bad row carrying the largest batch id
    is_bad = np.zeros(n, bool)
    is_bad[list(bad) + [640]] = True
    assert np.array_equal(is_bad, ((rows[:, :3] < 0) | (rows[:, :3] >= size)).any(1) | (rows[:, 3] < 0))
    d = torch.from_numpy(rows).to(DEV)
    keys = torch.zeros(n, dtype=torch.int64, device=DEV)
    vals = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    stats = torch.zeros(3, dtype=torch.int64, device=DEV)
    call("msp_point_keys", ptr(d), n, 6, log2, size, ptr(keys), ptr(vals), ptr(stats), _lib.stream())
    exp = R.morton_key(np.maximum(rows[:, 3], 0), *(np.clip(rows[:, i], 0, size - 1) for i in range(3)), log2)
    exp[is_bad] = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert np.array_equal(_u64(keys), exp)
    assert np.array_equal(_np(vals), np.arange(n, dtype=np.int32))
    n_desc = int((rows[1:, 3] < rows[:-1, 3]).sum())
    assert n_desc > 100
    assert _np(stats).tolist() == [int(is_bad.sum()), int(rows[~is_bad, 3].max()), n_desc]


def test_batch_starts_past_the_largest_id():
    """msp_batch_starts with n_batch greater than the largest id (ids {0, 1, 3}, n_batch = 7, row_stride 6):
    starts[b] is the lower bound of b; every b above 3 gives n."""
    rng = np.random.default_rng(5)
    n = 777
    rows = rng.integers(0, 50, (n, 6)).astype(np.int64)
    rows[:, 3] = np.sort(rng.choice([0, 1, 3], n))
    starts = torch.full((8,), -1, dtype=torch.int64, device=DEV)
    call("msp_batch_starts", ptr(torch.from_numpy(rows).to(DEV)), n, 6, 7, ptr(starts), _lib.stream())
    exp = np.searchsorted(rows[:, 3], np.arange(8), side="left")
    assert np.array_equal(_np(starts), exp)
    assert exp[2] == exp[3] and (exp[4:] == n).all()


# ---------------------------------------------------------------- 2. segment across the scan's edges
def _segment_keys(n, kind):
    rng = np.random.default_rng(n)
    if kind == "random":      # shift 0: a few duplicates; shift 3: ~n/1.6 groups; shift 6: ~n/8 groups
        return np.sort(rng.integers(0, 8 * n + 8, n)).astype(np.uint64)
    if kind == "equal":
        return np.full(n, 0x1234567, np.uint64)
    if kind == "distinct":    # distinct at every shift used
        return (np.arange(n, dtype=np.uint64) << np.uint64(6)) + np.uint64(5)
    assert kind == "edge2048"  # groups of 32 / 256 / 2048 rows at shift 0 / 3 / 6: boundaries exactly on row 2048
    i = np.arange(n, dtype=np.uint64)
    return ((i // np.uint64(2048)) << np.uint64(6)) + (i % np.uint64(2048)) // np.uint64(32)


@pytest.mark.parametrize("n,kind", [(n, k) for n in (1, 2047, 2048, 2049, 256 * 2048 + 2049)
                                    for k in ("random", "equal", "distinct")] +
                         [(3 * 2048, "edge2048"), (3 * 2048 + 7, "edge2048")])
def test_segment_direct(n, kind):
    """msp_segment called directly on sorted keys with shift 0, 3 and 6 against np.unique(keys >> shift).
    Scan path: scan_small_inplace, one block over ceil(n/2048) block sums -- 1 sum for n <= 2048, 2 for 2049,
    4 for the edge2048 cases, and 258 for n = 256*2048 + 2049, where the block's loop takes a second pass with
    a carry."""
    keys = _segment_keys(n, kind)
    assert (keys[1:] >= keys[:-1]).all()
    dk = torch.from_numpy(keys.view(np.int64)).to(DEV)
    perm_h = np.random.default_rng(1).permutation(n).astype(np.int32)
    perm = torch.from_numpy(perm_h).to(DEV)
    ws = torch.empty(((n + 2047) // 2048 + 1) * 8, dtype=torch.uint8, device=DEV)
    for shift in (0, 3, 6):
        seg_of = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        p2v = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        uniq = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        seg_start = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
        n_uniq = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        with_perm = shift == 0
        call("msp_segment", ptr(dk), n, shift, ptr(perm) if with_perm else None, ptr(seg_of),
             ptr(p2v) if with_perm else None, ptr(uniq), ptr(seg_start), ptr(n_uniq), ptr(ws), ws.numel(),
             _lib.stream())
        u, first, inv = np.unique(keys >> np.uint64(shift), return_index=True, return_inverse=True)
        G = len(u)
        assert int(n_uniq.item()) == G, (shift, int(n_uniq.item()), G)
        assert np.array_equal(_np(seg_of), inv.reshape(-1).astype(np.int32)), shift
        assert np.array_equal(_u64(uniq)[:G], u), shift
        assert np.array_equal(_np(seg_start)[:G + 1], np.append(first, n).astype(np.int32)), shift
        if with_perm:
            exp = np.empty(n, np.int32)
            exp[perm_h] = inv.reshape(-1)
            assert np.array_equal(_np(p2v), exp)
    if kind == "equal":
        assert G == 1
    if kind == "distinct":
        assert G == n


# ---------------------------------------------------------------- 3. neighbour map
@pytest.mark.parametrize("f", [1, 3, 5])
@pytest.mark.parametrize("name", ["full16", "corners4096", "sparse512", "sparse513", "one"])
def test_subm_map_entry_by_entry(name, f):
    """msp_hash_build + msp_subm_map_counted (through SubmRules) and msp_subm_map against subm_map, every entry.
    full16 has every site of both batches active: a neighbour past a face that is looked up instead of rejected
    lands on a present site (of the same batch or, the key space being contiguous, the next)."""
    b = _built(name)
    lvl = b["lvl"]
    V, K = lvl.n, f ** 3
    table, cap = lvl.hash()
    if name == "sparse512":
        assert V == 512 and cap == 1024, "cap == 2n exactly, the smallest legal table"
    if name == "sparse513":
        assert V == 513 and cap == 2048
    rules = metadata.SubmRules(lvl, f)
    nbr = _np(rules.nbr)[:, :V]
    exp = _ref_subm(name, f)
    assert nbr.shape == exp.shape == (K, V)
    assert np.array_equal(nbr, exp), f"{int((nbr != exp).sum())} wrong entries of {K * V}"
    assert rules.n_rules == int((exp >= 0).sum())
    assert np.array_equal(nbr[(K - 1) // 2], np.arange(V)), "the centre row is the identity"
    rows = np.arange(V)
    for o in range(K):
        p = nbr[o] >= 0
        assert np.array_equal(nbr[K - 1 - o][nbr[o][p]], rows[p]), f"offset {o} is not mirrored by {K - 1 - o}"
    plain = torch.full((K, V), -7, dtype=torch.int32, device=DEV)
    call("msp_subm_map", ptr(lvl.keys), V, lvl.log2, lvl.size, f, ptr(table), cap, ptr(plain), _lib.stream())
    assert np.array_equal(_np(plain), nbr), "msp_subm_map differs from msp_subm_map_counted"


# ---------------------------------------------------------------- 4. child map
def _check_down(fine_coords, coarse, rules, k):
    ref = R.down_map(fine_coords, k)
    n, Vc = len(fine_coords), len(ref["coarse"])
    assert coarse.n == Vc
    cc = ref["coarse"]
    exp_keys = R.morton_key(cc[:, 3], cc[:, 0], cc[:, 1], cc[:, 2], coarse.log2)
    assert np.array_equal(_u64(coarse.keys)[:Vc], exp_keys), "coarse keys"
    assert np.array_equal(_np(rules.parent_of)[:n].astype(np.int64), ref["parent_of"])
    assert np.array_equal(_np(rules.child_start).astype(np.int64), ref["child_start"])
    down = _np(rules.down)[:, :Vc]
    assert down.shape == ref["down"].shape == (8 ** k, Vc)
    assert np.array_equal(down, ref["down"]), f"{int((down != ref['down']).sum())} wrong entries"
    assert np.array_equal(np.sort(down[down >= 0]), np.arange(n)), "each fine row appears exactly once"
    return ref


@pytest.mark.parametrize("stride", [2, 4])
@pytest.mark.parametrize("name", ["full16", "corners4096", "single_child"])
def test_down_map_entry_by_entry(name, stride):
    """msp_segment with shift 3k and msp_down_map (through Metadata.downsample) against down_map: coarse keys,
    parent_of, child_start and every entry of down[8^k][Vc] (K = 64 for stride 4).  full16: every parent has all
    8^k children; single_child: every parent has one.  Scan path: one block, a single pass (<= 4 block sums)."""
    b = _built(name)
    k = stride.bit_length() - 1
    meta = metadata.Metadata(DEV)
    fine = meta.build_input(torch.from_numpy(b["coords"]), b["size"])
    coarse, rules = meta.downsample(b["size"], stride)
    assert coarse.size == b["size"] // stride and coarse.log2 == b["log2"] - k and rules.K == 8 ** k
    ref = _check_down(_np(meta.locations(b["size"])), coarse, rules, k)
    per_parent = np.diff(ref["child_start"])
    if name == "full16":
        assert (per_parent == 8 ** k).all() and (ref["down"] >= 0).all()
    if name == "single_child":
        assert (per_parent == 1).all() and coarse.n == fine.n
    assert np.array_equal(_np(meta.locations(coarse.size)), ref["coarse"]), "decoded coarse locations"


def test_down_map_stride_2_twice_equals_stride_4():
    """full16: 16 -> 8 -> 4 by two stride-2 steps gives the level that one stride-4 step gives, in one Metadata
    (the second arrival finds the level and keeps it) and in two."""
    b = _built("full16")
    coords = torch.from_numpy(b["coords"])
    one = metadata.Metadata(DEV)
    one.build_input(coords, 16)
    c4, r4 = one.downsample(16, 4)
    two = metadata.Metadata(DEV)
    two.build_input(coords, 16)
    c8, r2a = two.downsample(16, 2)
    c4b, r2b = two.downsample(8, 2)
    assert c4.n == c4b.n == 128 and c8.n == 1024
    assert np.array_equal(_u64(c4.keys)[:c4.n], _u64(c4b.keys)[:c4b.n])
    _check_down(_np(two.locations(8)), c4b, r2b, 1)
    # the stride-4 parent of a fine row is the stride-2 parent of its stride-2 parent
    p2 = _np(r2a.parent_of)[:8192].astype(np.int64)
    assert np.array_equal(_np(r2b.parent_of).astype(np.int64)[p2], _np(r4.parent_of)[:8192].astype(np.int64))
    # the same Metadata asked both ways keeps one level per size
    c8c, _ = one.downsample(16, 2)
    c4c, _ = one.downsample(8, 2)
    assert c4c is c4 and one.levels[4] is c4 and one.levels[8] is c8c and sorted(one.levels) == [4, 8, 16]


# ---------------------------------------------------------------- 5. pair lists
def _random_map(K, n, seed, absent=0.4, empty_offset=True):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 40000, (K, n)).astype(np.int32)
    m[rng.random((K, n)) < absent] = -1
    if empty_offset and K > 1:
        m[K // 2] = -1
    return m


@pytest.mark.parametrize("K,n", [(1, 1), (8, 2047), (8, 2048), (27, 2049), (64, 5000), (125, 40000)])
def test_pair_lists_entry_by_entry(K, n):
    """msp_pair_lists (count, then fill, through PairLists) against pair_lists(map): list order, an empty offset,
    n at the 2048-row block edge.  Scan path (scan_exclusive_i64 over K * ceil(n/2048) block counts): the
    one-tile kernel for 1, 8, 8, 54 and 192 counts; (125, 40000) has 2500 > 2048 counts -- the three-kernel
    scan (two blocks, then the block sums, then the apply)."""
    m = _random_map(K, n, K * 100003 + n)
    if (K, n) == (1, 1):
        m[0, 0] = 17
    dm = torch.from_numpy(m).to(DEV)
    pl = metadata.PairLists(dm, K, n, dm.device, _lib.stream())
    off_start, pin, pout = R.pair_lists(m)
    assert np.array_equal(_np(pl.off_start), off_start)
    assert pl.total == int(off_start[-1]) and pl.counts == np.diff(off_start).tolist()
    if K > 1:
        assert pl.counts[K // 2] == 0
    assert np.array_equal(_np(pl.pair_in)[:pl.total], pin)
    assert np.array_equal(_np(pl.pair_out)[:pl.total], pout)


@pytest.mark.parametrize("K,n", [(8, 2049), (125, 40000)])
def test_pair_lists_all_empty(K, n, monkeypatch):
    """An all -1 map: every start 0, total 0, and filling launches nothing (both scan paths)."""
    dm = torch.full((K, n), -1, dtype=torch.int32, device=DEV)
    pl = metadata.PairLists(dm, K, n, dm.device, _lib.stream())
    assert pl.total == 0 and pl.counts == [0] * K and pl.n_chunks == 0
    assert not _np(pl.off_start).any()
    launched = []
    real = metadata.call
    monkeypatch.setattr(metadata, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    assert pl.fill() is pl and pl.pair_in.numel() == 1 and pl.pair_out.numel() == 1
    assert "msp_pair_lists" not in launched


# ---------------------------------------------------------------- 6. tile rulebook
def _tile_rulebook_checked(m, K, n, T):
    dm = m if torch.is_tensor(m) else torch.from_numpy(m).to(DEV)
    rb = metadata.tile_rulebook(dm, K, n, dm.device, _lib.stream(), T)
    got = R.check_tile_rulebook(_np(dm), n, T, _np(rb["tile_start"]), _np(rb["chunk_off"]), _np(rb["chunk_src"]),
                                _np(rb["chunk_row"]))
    assert rb["n_chunks"] == got["n_chunks"] and rb["max_chunks"] == got["max_chunks"]
    return got


@pytest.mark.parametrize("K", [1, 27, 64, 125, 255])
@pytest.mark.parametrize("T", [64, 128, 256])
def test_tile_rulebook_forms(T, K):
    """msp_tile_rulebook at every tile size and K up to the ABI's 255 (K > 64: the per-wave scan of the chunk
    counts carries across 64-offset groups), n = 1000 (a partial last tile), 30 % absent, one offset empty.
    Scan path: the one-tile kernel with max_out (16, 8 or 4 tiles)."""
    got = _tile_rulebook_checked(_random_map(K, 1000, T * 1000 + K, absent=0.3), K, 1000, T)
    assert got["n_padding"] > 0


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_tile_rulebook_sizes(n):
    """T = 128, K = 27 around one tile: a single row, one row short of a tile, a full tile, one row into the
    second tile.  Scan path: the one-tile kernel (1 or 2 tiles)."""
    _tile_rulebook_checked(_random_map(27, n, n, absent=0.3, empty_offset=n > 1), 27, n, 128)


@pytest.mark.parametrize("per", [1, 16, 17, 128])
def test_tile_rulebook_density_edges(per):
    """T = 128, K = 27, five full tiles with exactly `per` present rows in every (tile, offset): 128 gives 8
    chunks per offset and no padding slot, 16 one full chunk, 17 one full chunk and one with 15 padding slots,
    and 1 a single present row, row 127 of the tile, owned by the second wave (padding takes its input row from
    there).  Scan path: the one-tile kernel."""
    K, T, nt = 27, 128, 5
    rng = np.random.default_rng(per)
    vals = rng.integers(0, 40000, (K, nt, T)).astype(np.int32)
    if per == 1:
        keep = np.zeros((K, nt, T), bool)
        keep[:, :, T - 1] = True
    else:
        keep = np.argsort(rng.random((K, nt, T)), axis=-1) < per
    assert (keep.sum(-1) == per).all()
    m = np.where(keep, vals, -1).reshape(K, nt * T).astype(np.int32)
    got = _tile_rulebook_checked(m, K, nt * T, T)
    chunks = -(-per // 16)
    assert got["n_chunks"] == K * nt * chunks and got["max_chunks"] == K * chunks
    assert got["n_padding"] == K * nt * (chunks * 16 - per)


def test_tile_rulebook_many_tiles():
    """T = 64, K = 2, n = 64 * 2049 + 5 at about 1/32 density: 2050 tiles > 2048, the scan's three-kernel path
    with max_out (block maxima reduced by the block-sum kernel); many tiles have an empty offset or none."""
    n = 64 * 2049 + 5
    rng = np.random.default_rng(2049)
    m = np.where(rng.random((2, n)) < 1 / 32, rng.integers(0, n, (2, n)), -1).astype(np.int32)
    got = _tile_rulebook_checked(m, 2, n, 64)
    assert got["max_chunks"] == 2 and got["n_chunks"] < 2 * 2050


def test_tile_rulebook_of_a_real_map():
    """corners4096's 3^3 neighbour map through SubmRules.tiles_for(128)."""
    lvl = _built("corners4096")["lvl"]
    rules = metadata.SubmRules(lvl, 3)
    rb = rules.tiles_for(128)
    assert lvl.n % 128 != 0
    got = R.check_tile_rulebook(_ref_subm("corners4096", 3), lvl.n, 128, _np(rb["tile_start"]),
                                _np(rb["chunk_off"]), _np(rb["chunk_src"]), _np(rb["chunk_row"]))
    assert rb["n_chunks"] == got["n_chunks"] and rb["max_chunks"] == got["max_chunks"]


# ---------------------------------------------------------------- 8. InputLayer averaging, heavy duplication
def test_input_layer_average_heavy_duplication():
    """scn.InputLayer(3, 16, mode=4) on 20 000 points of 8 channels, 15 000 of them in one voxel, N(3, 1) features
    (sums that do not cancel), against the fp64 per-voxel mean.

    Forward bound, per voxel: |err| <= count * 2^-24 * max|x| -- a sequential fp32 sum of `count` terms has error
    at most (count - 1) * 2^-24 * sum|x_i| to first order, the division adds 2^-24 * |mean|, and
    sum|x_i| / count <= max|x|.  Backward (msp_input_avg_bwd: each point gets grad / count, one fp32 division of
    an fp32 value by an exactly represented count): |err| <= 2^-23 * |ref|."""
    rng = np.random.default_rng(8)
    n, C, size = 20000, 8, 16
    coords = np.zeros((n, 4), np.int64)
    coords[:15000, :3] = (5, 9, 3)
    coords[15000:, :3] = rng.integers(0, size, (5000, 3))
    coords[15000:, 3] = rng.integers(0, 2, 5000)
    shuffle = rng.permutation(n)
    coords = coords[shuffle]
    x = (3.0 + rng.standard_normal((n, C))).astype(np.float32)
    feats = torch.from_numpy(x).to(DEV).requires_grad_(True)
    t = scn.InputLayer(3, size, mode=4)([torch.from_numpy(coords).to(DEV), feats])
    ref = R.voxelise(coords, 4)
    V = len(ref["keys"])
    to_ref = R.row_map(_np(t.metadata.locations(size)), R.decode_key(ref["keys"], 4), size)
    count = np.bincount(ref["p2v"], minlength=V)
    assert count.max() >= 15000 and (count == 1).any()
    x64 = x.astype(np.float64)
    mean = np.stack([np.bincount(ref["p2v"], weights=x64[:, c], minlength=V) for c in range(C)], 1) / count[:, None]
    amax = np.zeros(V)
    np.maximum.at(amax, ref["p2v"], np.abs(x64).max(1))
    got = _np(t.features).astype(np.float64)
    assert got.shape == (V, C)
    err = np.abs(got - mean[to_ref]).max(1)
    bound = (count * 2.0 ** -24 * amax)[to_ref]
    worst = int(np.argmax(err / bound))
    print(f"input avg fwd: largest err/bound {err[worst] / bound[worst]:.3e} at count {count[to_ref][worst]}; "
          f"the {count.max()}-point voxel: err {err[np.argmax(count[to_ref])]:.3e} "
          f"bound {bound[np.argmax(count[to_ref])]:.3e}")
    assert (err <= bound).all(), f"voxel of {count[to_ref][worst]} points: |err| {err[worst]:.3e} > {bound[worst]:.3e}"

    g = rng.standard_normal((V, C)).astype(np.float32)
    t.features.backward(torch.from_numpy(g).to(DEV))
    dev_row_of_point = np.empty(V, np.int64)
    dev_row_of_point[to_ref] = np.arange(V)
    v = dev_row_of_point[ref["p2v"]]                      # device voxel row of every point
    gref = g.astype(np.float64)[v] / count[to_ref][v][:, None]
    gerr = np.abs(_np(feats.grad).astype(np.float64) - gref)
    print(f"input avg bwd: largest err/|ref| {np.max(gerr / np.abs(gref)):.3e} (bound {2.0 ** -23:.3e})")
    assert (gerr <= 2.0 ** -23 * np.abs(gref)).all()
