"""The numpy restatements of tests/metadata_ref.py checked themselves (CPU): against oracle/scn_oracle.py, against
hand-worked answers, and -- for the rulebook checker -- against rulebooks that break one clause of the contract
each.  Also asserts that the clouds of tests/test_gpu_metadata.py hold the edges its tests rely on, so that a later
edit of a cloud cannot quietly remove them."""
import numpy as np
import pytest

import metadata_ref as R
import test_gpu_metadata as G
from oracle import scn_oracle as O
from wsss3d.synthetic import random_cloud


# ---------------------------------------------------------------- against the oracle
def _oracle_level(coords, size):
    _, first = np.unique(R.raster_key(coords, size), return_index=True)
    meta = O.OMeta()
    meta.levels[size] = O.OLevel(size, coords[first])
    return meta


def _cloud32():
    coords, _ = random_cloud(3000, 32, n_batch=2, seed=11, dense_frac=0.3)   # extent == size: the faces are hit
    assert coords[:, :3].min() == 0 and coords[:, :3].max() == 31
    return coords


def _by_second(a, b):
    order = np.lexsort((a, b))
    return a[order], b[order]


@pytest.mark.parametrize("f", [3, 5])
def test_subm_map_matches_oracle(f):
    coords, size = _cloud32(), 32
    lvl = _oracle_level(coords, size).levels[size]
    vox = R.decode_key(R.voxelise(coords, 5)["keys"], 5)        # the reference's own (Morton) row order
    assert len(vox) == lvl.n
    m = R.subm_map(vox, size, f)
    rk = R.raster_key(vox, size)
    total = 0
    for o, (oin, oout) in enumerate(lvl.subm_rules(f)):
        rows = np.nonzero(m[o] >= 0)[0]
        got = _by_second(rk[m[o][rows]], rk[rows])
        exp = _by_second(lvl.keys[oin], lvl.keys[oout])
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), f"offset {o}"
        total += len(rows)
    assert total > lvl.n      # not only the centre


@pytest.mark.parametrize("stride", [2, 4])
def test_down_map_matches_oracle(stride):
    coords, size = _cloud32(), 32
    k = stride.bit_length() - 1
    meta = _oracle_level(coords, size)
    csize, oparent, ooffset = meta.downsample(size, stride)
    fine, coarse = meta.levels[size], meta.levels[csize]
    vox = R.decode_key(R.voxelise(coords, 5)["keys"], 5)
    ref = R.down_map(vox, k)
    assert csize == size // stride and len(ref["coarse"]) == coarse.n
    o_idx, c_idx = np.nonzero(ref["down"] >= 0)
    rows = ref["down"][o_idx, c_idx]
    assert np.array_equal(np.sort(rows), np.arange(len(vox)))
    assert np.array_equal(ref["parent_of"][rows], c_idx)
    off_of = np.empty(len(vox), np.int64)
    off_of[rows] = o_idx
    to_oracle = R.row_map(vox, fine.coords, size)               # reference fine row -> oracle fine row
    assert np.array_equal(off_of, ooffset[to_oracle])
    assert np.array_equal(ref["coarse"][ref["parent_of"]], coarse.coords[oparent[to_oracle]])
    cs = ref["child_start"]
    assert cs[0] == 0 and cs[-1] == len(vox) and (np.diff(cs) >= 1).all()
    assert np.array_equal(np.repeat(np.arange(coarse.n), np.diff(cs)), ref["parent_of"])


def test_down_map_rejects_rows_out_of_key_order():
    vox = np.array([[0, 0, 0, 0], [2, 0, 0, 0], [1, 0, 0, 0]], np.int64)
    with pytest.raises(ValueError):
        R.down_map(vox, 1)


# ---------------------------------------------------------------- keys
def _decode_by_string(key, log2):
    """An independent decode: the key's binary digits dealt out as text."""
    key = int(key)
    bits = format(key & ((1 << (3 * log2)) - 1), f"0{3 * log2}b")
    return [int(bits[0::3], 2), int(bits[1::3], 2), int(bits[2::3], 2), key >> (3 * log2)]


def test_morton_key_round_trip_4096():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 4096, (300, 4))
    c[:, 3] = rng.integers(0, 9, 300)
    c[0] = (4095, 4095, 4095, 3)
    c[1] = (0, 0, 0, 0)
    c[2] = (4095, 0, 4095, 0)
    c[3] = (2048, 2047, 0, 1)
    keys = R.morton_key(c[:, 3], c[:, 0], c[:, 1], c[:, 2], 12)
    assert keys.dtype == np.uint64
    assert [_decode_by_string(k, 12) for k in keys] == c.tolist()
    assert np.array_equal(R.decode_key(keys, 12), c)
    assert int(keys[0]) == (3 << 36) | ((1 << 36) - 1) and int(keys[1]) == 0
    # hand-worked: x is the highest of the three interleaved bits, the batch id sits above 3 * log2
    assert [int(R.morton_key(0, *p, 12)) for p in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0))] == [4, 2, 1, 32]
    assert int(R.morton_key(1, 0, 0, 0, 12)) == 1 << 36 and int(R.morton_key(1, 0, 0, 0, 4)) == 1 << 12
    assert int(R.morton_key(0, 2048, 0, 0, 12)) == 1 << 35
    assert int(R.morton_key(0, 3, 5, 6, 3)) == 0b011_101_110 >> 0 and _decode_by_string(0b011101110, 3) == [3, 5, 6, 0]


def test_voxelise_by_hand():
    coords = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [1, 0, 0, 0]], np.int64)
    v = R.voxelise(coords, 2)
    assert v["keys"].tolist() == [1, 4, 64]
    assert v["p2v"].tolist() == [1, 0, 1, 2, 0, 1]
    assert v["vstart"].tolist() == [0, 2, 5, 6] and v["order"].tolist() == [1, 4, 0, 2, 5, 3]
    assert R.canonical_lists(np.array([4, 1, 5, 0, 2, 3]), v["vstart"]).tolist() == v["order"].tolist()
    assert R.canonical_lists(np.array([4, 0, 5, 1, 2, 3]), v["vstart"]).tolist() != v["order"].tolist()


def test_pair_lists_by_hand():
    m = np.array([[5, -1, 7], [-1, -1, -1], [0, 9, -1]], np.int32)
    off_start, pin, pout = R.pair_lists(m)
    assert off_start.tolist() == [0, 2, 2, 4] and pin.tolist() == [5, 7, 0, 9] and pout.tolist() == [0, 2, 0, 1]


# ---------------------------------------------------------------- the rulebook checker
def _build_rulebook(m, n, T):
    """A rulebook that meets the contract, built tile by tile; padding repeats the LAST present input row (any
    present row of the tile and offset is allowed)."""
    K = m.shape[0]
    n_tiles = (n + T - 1) // T
    tile_start, off, src, row = [0], [], [], []
    for t in range(n_tiles):
        chunks = 0
        for o in range(K):
            rows = np.nonzero(m[o, t * T:min(n, (t + 1) * T)] >= 0)[0]
            for c0 in range(0, len(rows), 16):
                part = rows[c0:c0 + 16]
                pad = 16 - len(part)
                off.append(o)
                src += m[o, t * T + part].tolist() + [int(m[o, t * T + rows[-1]])] * pad
                row += part.tolist() + [T] * pad
                chunks += 1
        tile_start.append(tile_start[-1] + chunks)
    tile_start.append(max(np.diff(tile_start)) if n_tiles else 0)
    return (np.array(tile_start, np.int64), np.array(off, np.uint8), np.array(src, np.int32),
            np.array(row, np.uint16).view(np.int16))


def _case(T=128, K=5, n=300, seed=0):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1000, (K, n)).astype(np.int32)
    m[rng.random((K, n)) < 0.3] = -1
    if K > 1:
        m[1] = -1
    return m, n, T


@pytest.mark.parametrize("T,K,n", [(64, 3, 200), (128, 5, 300), (256, 70, 600), (128, 2, 128), (64, 1, 1)])
def test_check_tile_rulebook_accepts_a_valid_rulebook(T, K, n):
    m, n, T = _case(T, K, n, seed=T + K)
    got = R.check_tile_rulebook(m, n, T, *_build_rulebook(m, n, T))
    assert got["n_chunks"] > 0 or n == 1


def test_check_tile_rulebook_accepts_an_empty_map():
    m = np.full((4, 100), -1, np.int32)
    ts = np.zeros(4, np.int64)
    assert R.check_tile_rulebook(m, 100, 64, ts, np.zeros(1, np.uint8), np.zeros(16, np.int32),
                                 np.zeros(16, np.int16))["n_chunks"] == 0
    ts[2] = 1
    with pytest.raises(AssertionError):
        R.check_tile_rulebook(m, 100, 64, ts, np.zeros(1, np.uint8), np.zeros(16, np.int32), np.zeros(16, np.int16))


def _break(name, m, n, T, ts, off, src, row):
    ts, off, src, row = ts.copy(), off.copy(), src.copy(), row.copy()
    pad = np.nonzero(row == T)[0]
    if name == "swapped entries":                    # storage order inside a chunk
        src[[0, 1]], row[[0, 1]] = src[[1, 0]], row[[1, 0]]
    elif name == "wrong input row":
        src[0] += 1
    elif name == "padding names an absent row":
        src[pad[0]] = 1001
    elif name == "padding from another offset":      # offset 0's first input row in a later offset's padding
        c = pad[-1] // 16
        assert off[c] != 0 and src[0] not in m[off[c]]
        src[pad[-1]] = src[0]
    elif name == "padding not marked":
        row[pad[0]] = T - 1
    elif name == "padding in the middle":
        c0 = (pad[0] // 16) * 16
        row[c0], src[c0] = T, src[c0 + 1]
    elif name == "offsets out of order":
        off[0], off[ts[1] - 1] = off[ts[1] - 1], off[0]
    elif name == "wrong total":
        ts[-2] += 1
    elif name == "wrong largest tile":
        ts[-1] -= 1
    elif name == "row past n":                       # the last tile is partial: rows 300..383 do not exist
        row[pad[-1]] = T - 1
    else:
        raise KeyError(name)
    return ts, off, src, row


@pytest.mark.parametrize("name", ["swapped entries", "wrong input row", "padding names an absent row",
                                  "padding from another offset", "padding not marked", "padding in the middle",
                                  "offsets out of order", "wrong total", "wrong largest tile", "row past n"])
def test_check_tile_rulebook_rejects(name):
    m, n, T = _case()
    good = _build_rulebook(m, n, T)
    R.check_tile_rulebook(m, n, T, *good)
    with pytest.raises(AssertionError):
        R.check_tile_rulebook(m, n, T, *_break(name, m, n, T, *good))


# ---------------------------------------------------------------- the GPU tests' clouds hold their edges
FACES = [(ax, side) for ax in range(3) for side in (0, 1)]


def _face_aliases(coords, size, f):
    """Per face: the (row, offset) entries whose neighbour lies outside the grid past that face and whose
    coordinates taken modulo the grid size are an active site of either batch."""
    vox = np.unique(coords, axis=0)
    out = {face: 0 for face in FACES}
    for d in R.offsets(f):
        q = vox.copy()
        q[:, :3] += d
        wrapped = q.copy()
        wrapped[:, :3] %= size
        active = np.zeros(len(vox), bool)
        for b in (0, 1):
            wrapped[:, 3] = b
            active |= R.lookup(vox, size, wrapped) >= 0
        for ax, side in FACES:
            past = q[:, ax] >= size if side else q[:, ax] < 0
            out[(ax, side)] += int((past & active).sum())
    return out


@pytest.mark.parametrize("f", [3, 5])
def test_full16_cloud_aliases_past_every_face(f):
    c = G.full16_cloud()
    assert c.shape == (16384, 4) and len(np.unique(c, axis=0)) == 8192
    assert not (np.diff(c[:, 3]) >= 0).all(), "shuffled"
    counts = _face_aliases(c, 16, f)
    assert all(v > 0 for v in counts.values()), counts
    # every site active: each out-of-grid neighbour of a face row aliases one (2 batches x 16^2 rows x f^2 x depth)
    assert counts[(0, 1)] == 2 * 256 * f * f * sum(range(1, f // 2 + 1))


def test_corners4096_cloud_edges():
    c = G.corners4096_cloud(True)
    s = G.corners4096_cloud(False)
    assert 5500 <= len(c) <= 6500
    assert np.array_equal(np.unique(c, axis=0), np.unique(s, axis=0)) and len(c) == len(s)
    assert (np.diff(c[:, 3]) >= 0).all() and not (np.diff(s[:, 3]) >= 0).all()
    assert sorted(set(c[:, 3].tolist())) == [0, 1, 3]
    vox = np.unique(c, axis=0)
    assert len(vox) < len(c), "duplicates"
    have = set(map(tuple, vox.tolist()))
    for ax in range(3):
        assert c[:, ax].min() == 0 and c[:, ax].max() == 4095
        for side in (0, 4095):                        # "points on each face", beyond the corners
            assert (c[:, ax] == side).sum() > 50
    for x in (0, 4095):
        for y in (0, 4095):
            for z in (0, 4095):
                assert (x, y, z, 0) in have and (x, y, z, 3) in have
    for lo in (0, 4080):                              # the two 16^3 blocks, about half occupied
        inside = ((vox[:, :3] >= lo) & (vox[:, :3] < lo + 16)).all(1) & (vox[:, 3] == 0)
        assert 0.4 * 4096 < inside.sum() < 0.6 * 4096
    # the slab on both sides of the top Morton bit of x
    assert ((vox[:, 0] == 2047) & (vox[:, 3] == 1)).any() and ((vox[:, 0] == 2048) & (vox[:, 3] == 1)).any()
    # adjacent active sites on both sides of a boundary of the 2(x) x 4(y) x 4(z) hash blocks, on every axis
    for ax, period in ((0, 2), (1, 4), (2, 4)):
        step = np.zeros(4, np.int64)
        step[ax] = 1
        last = vox[vox[:, ax] % period == period - 1]
        assert (R.lookup(vox, 4096, last + step) >= 0).sum() > 20, f"axis {ax}"
    # what a neighbour past a face of batch 0 would alias in batch 1 is there
    assert sum(_face_aliases(c, 4096, 3).values()) > 0
    assert len(vox) % 128 != 0                        # the real-map rulebook test wants a partial last tile


def test_sparse_and_single_child_clouds():
    for V in (512, 513):
        c = G.sparse_cloud(V)
        assert len(np.unique(c, axis=0)) == V and len(c) > V and c[:, :3].max() < 64
    assert G.one_cloud().tolist() == [[4095, 0, 4095, 0]]
    c = G.single_child_cloud()
    assert len(c) == 700 and len(np.unique(c, axis=0)) == 700
    for k in (1, 2):
        cc = c.copy()
        cc[:, :3] >>= k
        assert len(np.unique(cc, axis=0)) == 700
