"""Plain numpy restatements of the device metadata (csrc/msp_meta.hip), for tests only.

No torch, no device.  Every function restates the contract written in include/mi3dsparse.h in the most direct
form numpy offers -- bit loops, np.unique, np.searchsorted on raster keys, np.nonzero -- and none of them shares
a trick with the kernels (no magic-mask interleave, no block hash, no ballots, no scans).
tests/test_metadata_ref.py checks these restatements themselves against oracle/scn_oracle.py and by hand-built
cases; tests/test_gpu_metadata.py compares the kernels with them entry by entry.
"""
from __future__ import annotations

import numpy as np

CHUNK = 16  # MSP_CHUNK


# ---------------------------------------------------------------- keys
def morton_key(b, x, y, z, log2):
    """uint64 key: x at bit 3i+2, y at 3i+1, z at 3i for i < log2, batch id above bit 3*log2."""
    b, x, y, z = (np.asarray(v).astype(np.uint64) for v in (b, x, y, z))
    one = np.uint64(1)
    key = np.zeros(np.broadcast(b, x, y, z).shape, np.uint64)
    for i in range(int(log2)):
        s = np.uint64(i)
        key |= ((x >> s) & one) << np.uint64(3 * i + 2)
        key |= ((y >> s) & one) << np.uint64(3 * i + 1)
        key |= ((z >> s) & one) << np.uint64(3 * i)
    return key | (b << np.uint64(3 * int(log2)))


def decode_key(keys, log2):
    """(n, 4) int64 rows [x, y, z, b] of uint64 keys (the inverse of morton_key, again bit by bit)."""
    keys = np.asarray(keys).astype(np.uint64)
    one = np.uint64(1)
    out = np.zeros((len(keys), 4), np.int64)
    for i in range(int(log2)):
        out[:, 0] |= (((keys >> np.uint64(3 * i + 2)) & one) << np.uint64(i)).astype(np.int64)
        out[:, 1] |= (((keys >> np.uint64(3 * i + 1)) & one) << np.uint64(i)).astype(np.int64)
        out[:, 2] |= (((keys >> np.uint64(3 * i)) & one) << np.uint64(i)).astype(np.int64)
    out[:, 3] = (keys >> np.uint64(3 * int(log2))).astype(np.int64)
    return out


def voxelise(coords, log2):
    """coords (n, 4) [x, y, z, b] -> dict(keys, p2v, order, vstart).

    keys: the sorted distinct keys (one per voxel); p2v[i]: voxel of point i; the points of voxel v are
    order[vstart[v] : vstart[v + 1]], ascending."""
    coords = np.asarray(coords, np.int64)
    k = morton_key(coords[:, 3], coords[:, 0], coords[:, 1], coords[:, 2], log2)
    keys, p2v = np.unique(k, return_inverse=True)
    p2v = p2v.reshape(-1).astype(np.int64)
    order = np.argsort(p2v, kind="stable")
    vstart = np.concatenate([[0], np.cumsum(np.bincount(p2v, minlength=len(keys)))]).astype(np.int64)
    return dict(keys=keys, p2v=p2v, order=order, vstart=vstart)


def canonical_lists(perm, vstart):
    """perm with the entries of every run [vstart[v], vstart[v+1]) sorted ascending: two (perm, vstart) pairs
    describe the same per-voxel point sets iff vstart and this are equal."""
    perm = np.asarray(perm, np.int64)
    vstart = np.asarray(vstart, np.int64)
    seg = np.repeat(np.arange(len(vstart) - 1), np.diff(vstart))
    return perm[np.lexsort((perm, seg))]


# ---------------------------------------------------------------- lookups by raster key
def raster_key(c, size):
    c = np.asarray(c, np.int64)
    S = np.int64(size)
    return ((c[:, 3] * S + c[:, 0]) * S + c[:, 1]) * S + c[:, 2]


def lookup(vox_coords, size, query):
    """Row of every query coordinate row among vox_coords (distinct rows), or -1.  The bounds test is done on
    the coordinates, before any key is formed: an out-of-grid query never has a key."""
    vox_coords = np.asarray(vox_coords, np.int64)
    query = np.asarray(query, np.int64)
    keys = raster_key(vox_coords, size)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    ok = np.all((query[:, :3] >= 0) & (query[:, :3] < size), axis=1) & (query[:, 3] >= 0)
    out = np.full(len(query), -1, np.int64)
    if len(skeys) == 0 or not ok.any():
        return out
    qk = raster_key(query[ok], size)
    pos = np.minimum(np.searchsorted(skeys, qk), len(skeys) - 1)
    out[ok] = np.where(skeys[pos] == qk, order[pos], -1)
    return out


def row_map(from_coords, to_coords, size):
    """m with to_coords[m[r]] == from_coords[r]; both hold the same distinct rows."""
    m = lookup(to_coords, size, from_coords)
    assert len(from_coords) == len(to_coords) and (m >= 0).all() and len(np.unique(m)) == len(m), \
        "the two levels do not hold the same sites"
    return m


def offsets(f):
    """The f^3 offsets in map order: o = ((dx+h)*f + (dy+h))*f + (dz+h)."""
    h = f // 2
    r = np.arange(-h, h + 1)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def subm_map(vox_coords, size, f):
    """int32 [f^3][V]: row of the site at vox_coords[r] + offset o, or -1."""
    vox_coords = np.asarray(vox_coords, np.int64)
    V = len(vox_coords)
    out = np.full((f ** 3, V), -1, np.int32)
    for o, d in enumerate(offsets(f)):
        q = vox_coords.copy()
        q[:, :3] += d
        out[o] = lookup(vox_coords, size, q)
    return out


def down_map(vox_coords, log2_stride):
    """Strided relation of a level whose rows are in key order (children of a coarse site contiguous).

    -> dict(coarse (Vc, 4), parent_of [V], child_start [Vc + 1], down int32 [8^k][Vc]); coarse sites are numbered
    in order of first appearance, which for key-ordered rows is the coarse level's own key order."""
    c = np.asarray(vox_coords, np.int64)
    k = int(log2_stride)
    m = (1 << k) - 1
    cc = c.copy()
    cc[:, :3] >>= k
    uniq, first, inv = np.unique(cc, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    by_first = np.argsort(first, kind="stable")       # coarse sites by first fine row
    rank = np.empty(len(uniq), np.int64)
    rank[by_first] = np.arange(len(uniq))
    parent_of = rank[inv]
    if len(parent_of) and (np.diff(parent_of) < 0).any():
        raise ValueError("down_map: the children of a coarse site are not contiguous (rows not in key order)")
    Vc = len(uniq)
    child_start = np.searchsorted(parent_of, np.arange(Vc + 1), side="left").astype(np.int64)
    o = ((((c[:, 0] & m) << k) + (c[:, 1] & m)) << k) + (c[:, 2] & m)
    down = np.full((8 ** k, Vc), -1, np.int32)
    down[o, parent_of] = np.arange(len(c), dtype=np.int32)
    return dict(coarse=uniq[by_first], parent_of=parent_of, child_start=child_start, down=down)


# ---------------------------------------------------------------- pair lists
def pair_lists(m):
    """off_start [K + 1], pair_in, pair_out of an offset-major map: per offset, the present rows ascending."""
    m = np.asarray(m)
    K = m.shape[0]
    off_start = np.zeros(K + 1, np.int64)
    pin, pout = [], []
    for o in range(K):
        r = np.nonzero(m[o] >= 0)[0]
        pin.append(m[o][r].astype(np.int32))
        pout.append(r.astype(np.int32))
        off_start[o + 1] = off_start[o] + len(r)
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int32)  # noqa: E731
    return off_start, cat(pin), cat(pout)


# ---------------------------------------------------------------- tile rulebook
def check_tile_rulebook(m, n, T, tile_start, chunk_off, chunk_src, chunk_row):
    """Assert msp_tile_rulebook's contract (include/mi3dsparse.h) for the map m[K][n] and T-row tiles.

    The contract fixes everything but the value of a padding slot's chunk_src, so the expected chunk_off and
    chunk_row arrays and the expected non-padding chunk_src are built here and compared whole; a padding slot's
    chunk_src must be one of the present input rows of its tile and offset."""
    m = np.asarray(m)
    K = m.shape[0]
    assert m.ndim == 2 and m.shape[1] >= n, m.shape
    m = m[:, :n]
    n_tiles = (n + T - 1) // T
    tile_start = np.asarray(tile_start, np.int64)
    assert len(tile_start) >= n_tiles + 2, "tile_start holds n_tiles + 2 entries"
    # present[t][o][slot], rows past n absent
    padded = np.full((K, n_tiles * T), -1, np.int64)
    padded[:, :n] = m
    val = padded.reshape(K, n_tiles, T).transpose(1, 0, 2)             # [t][o][slot]
    present = val >= 0
    cnt = present.sum(-1)                                              # [t][o]
    nch = (cnt + CHUNK - 1) // CHUNK                                   # chunks of (tile, offset)
    per_tile = nch.sum(1)
    exp_start = np.concatenate([[0], np.cumsum(per_tile)]).astype(np.int64)
    total = int(exp_start[-1])
    assert np.array_equal(tile_start[:n_tiles + 1], exp_start), "tile_start: exclusive sums of ceil(present/16)"
    assert int(tile_start[n_tiles]) == total, "tile_start[n_tiles] is the chunk total"
    assert int(tile_start[n_tiles + 1]) == (int(per_tile.max()) if n_tiles else 0), \
        "tile_start[n_tiles + 1] is the largest per-tile chunk count"
    if total == 0:
        return dict(n_chunks=0, max_chunks=0, n_padding=0)

    chunk_off = np.asarray(chunk_off).astype(np.int64)[:total]
    chunk_src = np.asarray(chunk_src).astype(np.int64)[:total * CHUNK]
    chunk_row = np.asarray(chunk_row).astype(np.int64)[:total * CHUNK] & 0xFFFF   # uint16 in an int16 tensor
    assert len(chunk_off) == total and len(chunk_src) == total * CHUNK and len(chunk_row) == total * CHUNK

    # chunk order: tiles in order, inside a tile offsets ascending, ceil(present/16) chunks each
    flat_nch = nch.reshape(-1)                                         # (t, o) in storage order
    group_of_chunk = np.repeat(np.arange(n_tiles * K), flat_nch)
    tile_of_chunk = group_of_chunk // K
    same_tile = tile_of_chunk[1:] == tile_of_chunk[:-1]
    assert (np.diff(chunk_off)[same_tile] >= 0).all(), "chunk_off is non-decreasing over a tile's chunks"
    assert np.array_equal(chunk_off, group_of_chunk % K), \
        "each (tile, offset) has ceil(present/16) chunks, offsets ascending inside the tile"

    # expected entries: the present (slot, input row) of each (tile, offset), ascending slot, then padding
    chunk_base = np.concatenate([[0], np.cumsum(flat_nch)])[:-1]       # first chunk of (t, o)
    ent_base = np.concatenate([[0], np.cumsum(cnt.reshape(-1))])[:-1]  # first present entry of (t, o)
    t_i, o_i, s_i = np.nonzero(present)                                # (t, o, slot) order
    g_i = t_i * K + o_i
    rank = np.arange(len(g_i)) - ent_base[g_i]
    pos = chunk_base[g_i] * CHUNK + rank
    exp_row = np.full(total * CHUNK, T, np.int64)
    exp_src = np.full(total * CHUNK, -1, np.int64)
    exp_row[pos] = s_i
    exp_src[pos] = val[t_i, o_i, s_i]
    is_pad = exp_row == T
    assert np.array_equal(chunk_row == T, is_pad), \
        "padding (chunk_row == tile_rows) only at the tail of an offset's last chunk"
    assert np.array_equal(chunk_row, exp_row), "non-padding entries: the present rows of the tile, ascending"
    assert np.array_equal(chunk_src[~is_pad], exp_src[~is_pad]), "non-padding chunk_src is map[o][row]"
    rows = tile_of_chunk.repeat(CHUNK) * T + chunk_row
    assert (rows[~is_pad] < n).all(), "an entry names a row >= n"
    # padding repeats a present input row of the same tile and offset
    g_ent = group_of_chunk.repeat(CHUNK)
    have = np.unique(g_i.astype(np.int64) * (1 << 32) + exp_src[pos])
    want = g_ent[is_pad].astype(np.int64) * (1 << 32) + chunk_src[is_pad]
    assert (chunk_src[is_pad] >= 0).all() and np.isin(want, have).all(), \
        "a padding slot's chunk_src is not a present input row of its tile and offset"
    return dict(n_chunks=total, max_chunks=int(per_tile.max()), n_padding=int(is_pad.sum()))
