"""CPU builders and fp64 references for the convolution entries of include/mi3dsparse.h, for tests only.

numpy (and CPU torch in the moved rulebook checker); no device call.  Three parts:

  maps and rulebooks   make_map / make_single_map build offset-major maps [K][V] with the edges the kernels cut
                       at (tile, chunk and row-group sizes, empty tiles, empty offsets, tiles naming more distinct
                       rows than a staging buffer holds); tile_rulebook / local_rulebook / pair_rulebook /
                       dense_order restate the rulebook contracts of the header in loops.
  references           fwd / wgrad / pairs / epi_partial in fp64, straight from the map.
  data families        integer (|v| <= 3: every fp32 or split-bf16 evaluation is exact in any order; the builder
                       asserts sum |x||w| < 2^24), pieces-x / pieces-w (24-bit mantissas on one side, a selector of
                       0 / +-2^e on the other, at most one non-zero term per output element -- asserted -- so the
                       result is exact and is wrong when a kernel drops or misroutes the second or third bf16
                       piece), normal (as tests/test_gpu_ops.py draws them).

The case lists of tests/test_gpu_conv_forms.py live here too (tile_cases() ... narrow_cases()), so that tests/test_conv_ref.py checks on
the CPU what the GPU file relies on.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

import metadata_ref as MR

F32, F64 = np.float32, np.float64
T = 128            # rows of a tile (msp_conv_tile_rows)
CHUNK = 16         # MSP_CHUNK
X6S_STAGE = 383    # distinct rows a tile-local tile stages in LDS (msp_conv_local)
RAGGED = (0, 1, 15, 16, 17, 127, 128)
ROWS = (1, 15, 16, 17, 127, 128, 129, 257, 1023, 1025)
FAMILY_ROWS = (1, 129, 1025)
EXACT = ("integer", "pieces-x", "pieces-w")


# ---------------------------------------------------------------- maps
def _rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def injective_per_offset(m):
    """Every input row is named at most once by each offset."""
    for o in range(m.shape[0]):
        v = m[o][m[o] >= 0]
        if len(np.unique(v)) != len(v):
            return False
    return True


def cloud(V, seed):
    """V distinct sites [x, y, z, 0] of a box filled to about 30 %, rows in Morton order."""
    rng = _rng(V, seed, 41)
    side = max(2, int(np.ceil((V / 0.3) ** (1 / 3))))
    cells = np.sort(rng.choice(side ** 3, V, replace=False))
    c = np.stack([cells // (side * side), (cells // side) % side, cells % side, np.zeros_like(cells)], 1).astype(np.int64)
    return c[np.argsort(MR.morton_key(c[:, 3], c[:, 0], c[:, 1], c[:, 2], 6), kind="stable")], 64


def _ragged(K, V, n_in, seed, hole):
    assert n_in >= V
    rng = _rng(K, V, n_in, seed, 43)
    m = np.full((K, V), -1, np.int32)
    n_tiles = -(-V // T)
    pool = [rng.permutation(n_in) for _ in range(K)]       # each offset hands its rows out once
    used = [0] * K
    for t in range(n_tiles):
        rows_t = min(T, V - t * T)
        if hole and n_tiles >= 2 and (t == n_tiles // 2 or t == n_tiles - 1):
            continue
        for o in range(K):
            cnt = min(RAGGED[(t * K + o + seed) % len(RAGGED)], rows_t)
            rows = np.sort(rng.choice(rows_t, cnt, replace=False)) + t * T
            m[o, rows] = pool[o][used[o]:used[o] + cnt]
            used[o] += cnt
    return m


def _wide(K, V, n_in, seed):
    assert K >= 4 and V > 2 * T and n_in >= 20000
    rng = _rng(K, V, n_in, seed, 47)
    m = rng.integers(0, n_in, (K, V)).astype(np.int32)
    m[rng.random((K, V)) < 0.3] = -1
    for t, want in ((0, X6S_STAGE), (1, X6S_STAGE + 1)):   # exactly the stage's size, and one more
        blk = m[:, t * T:(t + 1) * T]
        o_i, r_i = np.nonzero(blk >= 0)
        assert len(o_i) >= want
        names = rng.choice(n_in, want, replace=False)
        vals = np.concatenate([names, rng.choice(names, len(o_i) - want)])
        p = rng.permutation(len(o_i))
        blk[o_i[p], r_i[p]] = vals
    return m


@functools.lru_cache(maxsize=None)
def make_map(kind, K, V, n_in=None, seed=0):
    """int32 [K][V] map into n_in input rows, -1 absent -> (map, n_in).  `cloud_down` takes V as the number of
    fine (input) rows and returns the map over however many coarse rows they have."""
    if kind == "centre":
        n_in = V if n_in is None else n_in
        m = np.full((K, V), -1, np.int32)
        m[K // 2] = _rng(K, V, seed, 53).permutation(n_in)[:V]
    elif kind == "full":
        n_in = V if n_in is None else n_in
        rng = _rng(K, V, seed, 59)
        m = np.stack([rng.permutation(n_in)[:V] for _ in range(K)]).astype(np.int32)
    elif kind in ("ragged", "hole"):
        n_in = V + 3 if n_in is None else n_in
        m = _ragged(K, V, n_in, seed, kind == "hole")
    elif kind == "wide":
        n_in = 50000 if n_in is None else n_in
        m = _wide(K, V, n_in, seed)
    elif kind == "cloud3":
        assert K == 27
        c, size = cloud(V, seed)
        m, n_in = MR.subm_map(c, size, 3), V
    elif kind == "cloud_down":
        assert K == 8
        c, _ = cloud(V, seed)
        m, n_in = MR.down_map(c, 1)["down"], V
        assert m.shape[1] != n_in
    else:
        raise ValueError(kind)
    m = np.ascontiguousarray(m, np.int32)
    assert m.shape[0] == K and ((m >= -1) & (m < n_in)).all()
    if kind != "wide":
        assert injective_per_offset(m), kind
    else:
        d = [len(np.unique(m[:, t * T:(t + 1) * T][m[:, t * T:(t + 1) * T] >= 0])) for t in range(-(-V // T))]
        assert d[0] == X6S_STAGE and d[1] == X6S_STAGE + 1 and max(d[2:]) > 2 * X6S_STAGE, d
    m.setflags(write=False)
    return m, n_in


@functools.lru_cache(maxsize=None)
def make_single_map(counts, n_in, seed=0):
    """A map whose every row has exactly one offset (the pair-list entries' one contribution per output row):
    offset o owns counts[o] rows, dealt at random; every input row is named at most once over all offsets."""
    counts = tuple(int(c) for c in counts)
    K, V = len(counts), sum(counts)
    assert n_in >= V
    rng = _rng(K, V, n_in, seed, 61)
    rows, src = rng.permutation(V), rng.permutation(n_in)[:V]
    m = np.full((K, V), -1, np.int32)
    s = 0
    for o, c in enumerate(counts):
        m[o, rows[s:s + c]] = src[s:s + c]
        s += c
    assert ((m >= 0).sum(0) == 1).all() and len(np.unique(m[m >= 0])) == V
    m.setflags(write=False)
    return m, n_in


# ---------------------------------------------------------------- rulebooks
def tile_rulebook(m, tile_rows=T):
    """msp_tile_rulebook's contract: per tile, per offset ascending, the present (row, input row) entries in
    16-entry chunks; a padding slot has chunk_row = tile_rows and repeats the group's first input row."""
    K, V = m.shape
    n_tiles = -(-V // tile_rows)
    tile_start = np.zeros(n_tiles + 2, np.int64)
    off, src, row = [], [], []
    for t in range(n_tiles):
        blk = m[:, t * tile_rows:(t + 1) * tile_rows]
        n0 = len(off)
        for o in range(K):
            r = np.nonzero(blk[o] >= 0)[0]
            for c0 in range(0, len(r), CHUNK):
                rc = r[c0:c0 + CHUNK]
                pad = CHUNK - len(rc)
                off.append(o)
                src.append(np.concatenate([blk[o][rc], np.full(pad, blk[o][r[0]])]))
                row.append(np.concatenate([rc, np.full(pad, tile_rows)]))
        tile_start[t + 1] = len(off)
        tile_start[n_tiles + 1] = max(tile_start[n_tiles + 1], len(off) - n0)
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)  # noqa: E731
    return dict(tile_rows=tile_rows, n_tiles=n_tiles, tile_start=tile_start, chunk_off=np.asarray(off, np.uint8),
                chunk_src=cat(src, np.int32), chunk_row=cat(row, np.uint16), n_chunks=len(off))


def local_rulebook(m, shuffle=None, wave_off=True, tile_rows=T):
    """msp_tile_local's contract: u_rows (sorted distinct input rows per tile), u_start [n_tiles + 2], perm (the
    tile's rows, identity or -- shuffle = a seed -- shuffled inside each tile; -1 past V), lidx [K][n_tiles * T]
    (position in the tile's list, 0xFFFF none) and wave_off (per row half the offsets some row of the half has,
    each once, dealt onto the 4 waves; 0xFF none) or None."""
    K, V = m.shape
    n_tiles = -(-V // tile_rows)
    n_pad = n_tiles * tile_rows
    perm = np.full(n_pad, -1, np.int32)
    lidx = np.full((K, n_pad), 0xFFFF, np.uint16)
    u_start = np.zeros(n_tiles + 2, np.int64)
    u_rows = []
    wo = np.full(n_tiles * 64, 0xFF, np.uint8)
    rng = None if shuffle is None else _rng(K, V, shuffle, 67)
    for t in range(n_tiles):
        rows = np.arange(t * tile_rows, min((t + 1) * tile_rows, V))
        if rng is not None:
            rows = rng.permutation(rows)
        perm[t * tile_rows:t * tile_rows + len(rows)] = rows
        ent = m[:, rows]
        u = np.unique(ent[ent >= 0])
        assert len(u) < 0xFFFF
        u_rows.append(u)
        u_start[t + 1] = u_start[t] + len(u)
        u_start[n_tiles + 1] = max(u_start[n_tiles + 1], len(u))
        li = np.where(ent >= 0, np.searchsorted(u, np.maximum(ent, 0)), 0xFFFF)
        lidx[:, t * tile_rows:t * tile_rows + len(rows)] = li
        if wave_off:
            has = np.zeros((K, tile_rows), bool)
            has[:, :len(rows)] = ent >= 0
            grp = has.reshape(K, tile_rows // 16, 16).any(2)
            for h in range(2):
                need = [o for o in range(K) if grp[o, h::2].any()]
                need.sort(key=lambda o: -int(has[o].sum()))
                fill = [0] * 4
                for o in need:
                    c = int(np.argmin(fill))
                    assert fill[c] < 8
                    wo[t * 64 + h * 32 + c * 8 + fill[c]] = o
                    fill[c] += 1
    u_rows = np.concatenate(u_rows).astype(np.int32) if u_rows else np.zeros(0, np.int32)
    ok = wave_off and tile_rows == 128 and K <= 27
    return dict(tile_rows=tile_rows, n_tiles=n_tiles, u_start=u_start, u_rows=u_rows, perm=perm, lidx=lidx,
                wave_off=wo if ok else None, total=int(u_start[n_tiles]), max_u=int(u_start[n_tiles + 1]))


def pair_rulebook(m, swap=False):
    """metadata_ref.pair_lists plus chunk_start [K + 1] = prefix sums of ceil(n_o / 16).  swap: the pairs run
    from the map's rows to the rows it names (deconvolution forward over a child map)."""
    off_start, pin, pout = MR.pair_lists(m)
    if swap:
        pin, pout = pout, pin
    n_o = np.diff(off_start)
    chunk_start = np.concatenate([[0], np.cumsum(-(-n_o // CHUNK))]).astype(np.int64)
    return dict(off_start=off_start, pair_in=pin, pair_out=pout, chunk_start=chunk_start,
                n_chunks=int(chunk_start[-1]), total=int(off_start[-1]))


def dense_order(m, seed=0):
    """A row order for msp_conv_nbr: perm (position j is output row perm[j]) and the permuted map."""
    perm = _rng(m.shape[0], m.shape[1], seed, 71).permutation(m.shape[1]).astype(np.int32)
    return perm, np.ascontiguousarray(m[:, perm])


def _t(a):
    import torch
    if isinstance(a, torch.Tensor):
        return a.cpu()
    a = np.asarray(a)
    if a.dtype == np.uint16:
        a = a.astype(np.int64)
    return torch.from_numpy(np.array(a))


def check_local_rulebook(nbr, loc, n):
    """Assert msp_tile_local's contract for the map nbr [K][n]; loc holds device tensors (the library's
    rulebook) or numpy arrays (local_rulebook above)."""
    import torch
    nbr = _t(nbr)
    K = nbr.size(0)
    T, nt = loc["tile_rows"], loc["n_tiles"]
    us = _t(loc["u_start"])[:nt + 1]
    u_rows = _t(loc["u_rows"])
    perm = _t(loc["perm"])[:nt * T].view(nt, T)
    lidx = _t(loc["lidx"])[:, :nt * T].to(torch.int64) & 0xFFFF  # uint16 bits in an int16 tensor
    nb = nbr
    assert loc["total"] == int(us[-1]) and loc["max_u"] == int((us[1:] - us[:-1]).max())
    for t in range(nt):
        rows = perm[t]
        valid = rows >= 0
        assert int(valid.sum()) == min(T, n - t * T)
        assert bool((~valid[int(valid.sum()):]).all())  # padding last
        assert sorted(rows[valid].tolist()) == list(range(t * T, t * T + int(valid.sum())))
        u = u_rows[int(us[t]):int(us[t + 1])]
        assert bool((u[1:] > u[:-1]).all())
        ent = nb[:, rows[valid].long()]
        assert sorted(set(ent[ent >= 0].tolist())) == u.tolist()
        li = lidx[:, t * T:(t + 1) * T][:, :int(valid.sum())]
        absent = ent < 0
        assert bool((li[absent] == 0xFFFF).all())
        assert torch.equal(u[li[~absent]], ent[~absent])
    wo = loc.get("wave_off")
    if T == 128 and K <= 27:  # conv_x6s's offset lists: per half, every offset some row has, once, packed
        wo = _t(wo)[:nt * 64].view(nt, 2, 4, 8).to(torch.int64)
        has = torch.zeros(K, nt * T, dtype=torch.bool)
        for t in range(nt):
            rows = perm[t]
            has[:, t * T:t * T + int((rows >= 0).sum())] = nb[:, rows[rows >= 0].long()] >= 0
        has = has.view(K, nt, T // 16, 16).any(3)  # [K][tile][group]
        for t in range(nt):
            for h in range(2):
                need = sorted(o for o in range(K) if bool(has[o, t, h::2].any()))
                lists = wo[t, h]
                got = []
                for c in range(4):
                    n = int((lists[c] != 0xFF).sum())
                    assert bool((lists[c, :n] != 0xFF).all()) and bool((lists[c, n:] == 0xFF).all())
                    got += lists[c, :n].tolist()
                assert sorted(got) == need, (t, h)
    else:
        assert wo is None


# ---------------------------------------------------------------- references (fp64)
def weight_matrices(w, flip):
    """[K][c_in][c_out] fp64, indexed by the MAP's offset, of weights given as the kernels take them: flip bit 1
    set: w is [K][c_in][c_out], else [K][c_out][c_in]; bit 0: offset o reads w[K - 1 - o]; bit 2 changes no
    value (the workspace already holds the split image)."""
    W = np.asarray(w, F64)
    if not flip & 2:
        W = W.transpose(0, 2, 1)
    return W[::-1] if flip & 1 else W


def kernel_weights(Wm, flip):
    """The inverse: float32 weights in the layout a call with `flip` takes, from [K][c_in][c_out] by map offset."""
    W = Wm[::-1] if flip & 1 else Wm
    if not flip & 2:
        W = W.transpose(0, 2, 1)
    return np.ascontiguousarray(W, F32)


def fwd(x, w, m, flip):
    """out[r] = sum_o x[m[o][r]] W(o), fp64 [V][c_out]."""
    Wm = weight_matrices(w, flip)
    x64 = np.asarray(x, F64)
    out = np.zeros((m.shape[1], Wm.shape[2]), F64)
    for o in range(m.shape[0]):
        r = np.nonzero(m[o] >= 0)[0]
        if len(r):
            out[r] += x64[m[o][r]] @ Wm[o]
    return out


def fwd_tiles(x, w, tl, V, flip):
    """The same sum taken from a tile rulebook, entry by entry (checks a rulebook against its map)."""
    Wm = weight_matrices(w, flip)
    x64 = np.asarray(x, F64)
    out = np.zeros((V, Wm.shape[2]), F64)
    Tr = tl["tile_rows"]
    for t in range(tl["n_tiles"]):
        for c in range(int(tl["tile_start"][t]), int(tl["tile_start"][t + 1])):
            for j in range(CHUNK):
                rr = int(tl["chunk_row"][c * CHUNK + j])
                if rr < Tr:
                    out[t * Tr + rr] += x64[tl["chunk_src"][c * CHUNK + j]] @ Wm[tl["chunk_off"][c]]
    return out


def wgrad(x, dy, m):
    """dW[o][ci][co] = sum over rows r with m[o][r] >= 0 of x[m[o][r]][ci] dy[r][co], fp64."""
    x64, d64 = np.asarray(x, F64), np.asarray(dy, F64)
    dw = np.zeros((m.shape[0], x64.shape[1], d64.shape[1]), F64)
    for o in range(m.shape[0]):
        r = np.nonzero(m[o] >= 0)[0]
        if len(r):
            dw[o] = x64[m[o][r]].T @ d64[r]
    return dw


def pairs(x, wt, pin, pout, off_start, n_out):
    """out[pout[p]] = wt[o] x[pin[p]] for the pairs of offset o (wt [K][c_out][c_in]); rows no pair names NaN."""
    x64, W = np.asarray(x, F64), np.asarray(wt, F64)
    out = np.full((n_out, W.shape[1]), np.nan, F64)
    for o in range(W.shape[0]):
        s, e = int(off_start[o]), int(off_start[o + 1])
        out[pout[s:e]] = x64[pin[s:e]] @ W[o].T
    return out


def epi_partial(out32, tile_rows=T):
    """The forward epilogue's buffer partial[2][C][P]: per 128-row tile (sum v, sum v^2) of the fp32 output."""
    V, C = out32.shape
    P = -(-V // tile_rows)
    v = np.zeros((P * tile_rows, C), F64)
    v[:V] = out32
    v = v.reshape(P, tile_rows, C)
    return np.stack([v.sum(1).T, (v * v).sum(1).T])


# ---------------------------------------------------------------- data families
def _ints(rng, shape):
    return rng.integers(-3, 4, shape).astype(F32)


def _wide_values(rng, shape):
    """Full 24-bit mantissas (lowest bit set: the third bf16 piece is never zero), magnitudes in [2^-8, 2^8)."""
    mant = (rng.integers(0, 1 << 23, shape) | 1).astype(F64) / (1 << 23) + 1.0
    v = mant * np.exp2(rng.integers(-8, 8, shape).astype(F64)) * rng.choice([-1.0, 1.0], shape)
    out = v.astype(F32)
    assert np.array_equal(out.astype(F64), v)
    return out


def _pow2(rng, shape):
    return (np.exp2(rng.integers(-4, 5, shape).astype(F64)) * rng.choice([-1.0, 1.0], shape)).astype(F32)


def _rows_seen_once(m, n_in, rng, limit=4096):
    """Input rows such that no output row sees two of them (or one of them twice), greedily."""
    o_i, r_i = np.nonzero(m >= 0)
    j = m[o_i, r_i]
    order = np.argsort(j, kind="stable")
    j_s, r_s = j[order], r_i[order]
    starts = np.searchsorted(j_s, np.arange(n_in + 1))
    hit = np.zeros(m.shape[1], bool)
    chosen = []
    cand = np.unique(j_s)
    for c in rng.permutation(cand)[:limit]:
        rs = r_s[starts[c]:starts[c + 1]]
        if len(np.unique(rs)) < len(rs) or hit[rs].any():
            continue
        hit[rs] = True
        chosen.append(c)
    return np.asarray(chosen, np.int64)


def fwd_data(family, m, n_in, c_in, c_out, flip, seed=0, per_offset=False):
    """x [n_in][c_in] and w (as a call with `flip` takes it) of one family, with the family's property asserted.
    per_offset: the pieces-x selector picks one input channel per (offset, output channel) instead of one (offset,
    input channel) per output channel -- for maps whose rows have one offset each."""
    K = m.shape[0]
    rng = _rng(family, K, m.shape[1], n_in, c_in, c_out, flip, seed)
    if family == "integer":
        x, Wm = _ints(rng, (n_in, c_in)), _ints(rng, (K, c_in, c_out))
        x[0] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], c_in)   # a kernel reading row 0 for "absent" shows
    elif family == "pieces-x":
        x = _wide_values(rng, (n_in, c_in))
        Wm = np.zeros((K, c_in, c_out), F32)
        co = np.arange(c_out)
        if per_offset:
            for o in range(K):
                Wm[o, rng.integers(0, c_in, c_out), co] = _pow2(rng, c_out)
        else:
            Wm[rng.integers(0, K, c_out), rng.integers(0, c_in, c_out), co] = _pow2(rng, c_out)
    elif family == "pieces-w":
        Wm = _wide_values(rng, (K, c_in, c_out))
        x = np.zeros((n_in, c_in), F32)
        rows = _rows_seen_once(m, n_in, rng)
        x[rows, rng.integers(0, c_in, len(rows))] = _pow2(rng, len(rows))
    elif family == "normal":
        x = rng.standard_normal((n_in, c_in)).astype(F32)
        Wm = (rng.standard_normal((K, c_in, c_out)) / (K * c_in) ** 0.5).astype(F32)
    else:
        raise ValueError(family)
    w = kernel_weights(Wm, flip)
    if family == "integer":
        assert fwd(np.abs(x), np.abs(w), m, flip).max(initial=0) < 1 << 24
    elif family in EXACT:
        assert fwd(x != 0, w != 0, m, flip).max(initial=0) <= 1, "more than one non-zero term in an output element"
    return x, w


def wgrad_data(family, m, n_in, c_in, c_out, seed=0):
    """x [n_in][c_in] and dy [V][c_out] of one family for a weight gradient over the map."""
    K, V = m.shape
    rng = _rng(family, K, V, n_in, c_in, c_out, seed, 73)
    named = np.unique(m[m >= 0]) if (m >= 0).any() else np.zeros(1, np.int64)
    if family == "integer":
        x, dy = _ints(rng, (n_in, c_in)), _ints(rng, (V, c_out))
        x[0] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], c_in)
    elif family == "pieces-x":     # each dy column is non-zero in one row
        x = _wide_values(rng, (n_in, c_in))
        dy = np.zeros((V, c_out), F32)
        live = np.nonzero((m >= 0).any(0))[0] if (m >= 0).any() else np.zeros(1, np.int64)
        dy[rng.choice(live, c_out), np.arange(c_out)] = _pow2(rng, c_out)
    elif family == "pieces-w":     # each x column is non-zero in one input row
        dy = _wide_values(rng, (V, c_out))
        x = np.zeros((n_in, c_in), F32)
        x[rng.choice(named, c_in), np.arange(c_in)] = _pow2(rng, c_in)
    elif family == "normal":
        x = rng.standard_normal((n_in, c_in)).astype(F32)
        dy = rng.standard_normal((V, c_out)).astype(F32)
    else:
        raise ValueError(family)
    if family == "integer":
        assert wgrad(np.abs(x), np.abs(dy), m).max(initial=0) < 1 << 24
    elif family in EXACT:
        assert wgrad(x != 0, dy != 0, m).max(initial=0) <= 1, "more than one non-zero term in a dW element"
    return x, dy


# ---------------------------------------------------------------- comparisons
def compare_exact(got, ref64, what=""):
    """got (fp32) must equal the fp64 reference rounded to fp32, element by element (NaN equals NaN)."""
    got = np.asarray(got)
    exp = np.asarray(ref64, F64).astype(F32)
    assert got.dtype == F32 and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    bad = ~((got == exp) | (np.isnan(got) & np.isnan(exp)))
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {i}: "
                             f"got {got[i]!r}, expected {exp[i]!r}")


def rel_err(got, ref64):
    """(max |got - ref| / max |ref|, max |ref|)."""
    ref64 = np.asarray(ref64, F64)
    scale = float(np.abs(ref64).max(initial=0)) or 1.0
    return float(np.abs(np.asarray(got, F64) - ref64).max(initial=0)) / scale, scale


def compare_bar(got, ref64, mult, plain32=None, what=""):
    """The bars tests/test_gpu_ops.py states.  mult 3 (x6d, x6r) / 2 (conv_nbr): error <= max(mult x the error of
    a plain fp32 evaluation, 1e-7) and < 1e-6 of the output scale; mult None with plain32 None: < 1e-6 (conv_local,
    chunk weight gradient); mult "f32": 1e-5 (the f32 forms, the pair-list weight gradient)."""
    err, _ = rel_err(got, ref64)
    if mult == "f32":
        bound = 1e-5
        ok = err < bound
    elif mult is None:
        bound = 1e-6
        ok = err < bound
    else:
        e32, _ = rel_err(plain32, ref64)
        bound = min(max(mult * e32, 1e-7), 1e-6)
        ok = err <= max(mult * e32, 1e-7) and err < 1e-6
    print(f"{what}: worst error {err:.3e} of the output scale, bound {bound:.3e}")
    assert ok, (what, err, bound)
    return err, bound


def plain_fp32(x, w, m, flip):
    """A plain fp32 evaluation of fwd (gather + fp32 matrix product per offset, fp32 accumulation)."""
    W = np.asarray(w, F32)
    if not flip & 2:
        W = W.transpose(0, 2, 1)
    if flip & 1:
        W = W[::-1]
    out = np.zeros((m.shape[1], W.shape[2]), F32)
    for o in range(m.shape[0]):
        r = np.nonzero(m[o] >= 0)[0]
        if len(r):
            out[r] += np.asarray(x, F32)[m[o][r]] @ W[o]
    return out


# ---------------------------------------------------------------- the dispatch, restated (csrc/msp_conv*.hip)
def use_x6r(V, c_in, c_out):
    return (c_out <= 32 and c_in <= 64) or (c_out == 64 and c_in <= 32 and V >= 100000)


def plan_x6(V, c_out):
    """(nt, nb, n_y, split) of the shared-tile form."""
    n16, n_tiles = c_out // 16, -(-V // T)
    nt, nb = 1, 2
    if n16 % 4 == 0 and n_tiles * (n16 // 4) >= 256:
        nt, nb = 4, 1
    else:
        for c in (3, 4, 2):
            if n16 % c == 0:
                nt = c
                break
    n_y = n16 // nt
    blocks = n_tiles * n_y
    target, cap = (2048, 16) if n_tiles <= 8 else (1024, 8)
    split = min(cap, -(-target // blocks)) if blocks < target else 1
    return nt, nb, n_y, split


def round256(b):
    return (b + 255) & ~255


def tile_ws_bytes(V, K, c_in, c_out):
    c_pad = -(-c_in // 32) * 32
    if use_x6r(V, c_in, c_out):
        return K * c_out * c_pad * 6
    split = plan_x6(V, c_out)[3]
    return round256(K * 3 * c_out * c_pad * 2) + (split * V * c_out * 4 if split > 1 else 0)


def x6r_form(c_in, c_out):
    """launch_x6r's (NT x 16 columns, NKK x 32 input channels)."""
    n16 = c_out // 16
    return (32 if n16 >= 2 and n16 % 2 == 0 else 16), 32 * (-(-c_in // 32))


def tile_form_id(V, c_in, c_out):
    if use_x6r(V, c_in, c_out):
        nc, kk = x6r_form(c_in, c_out)
        return f"x6r-NT{nc // 16}-NKK{kk // 32}" + ("-2pass" if c_out == 64 else "")
    nt, nb, n_y, split = plan_x6(V, c_out)
    return f"x6d-nt{nt}-nb{nb}-ny{n_y}-split{split}"


def local_nt(c_out):
    return 2 if (c_out // 16) % 2 == 0 else 1


def pick_tile(n16):
    return 4 if n16 % 4 == 0 else 3 if n16 % 3 == 0 else 2 if n16 % 2 == 0 else 1


def pairs_form_id(n_chunks, c_in, c_out):
    """msp_conv_pairs: register runs for c_in <= 64 (run length from the chunk count), else one chunk per wave."""
    nt = pick_tile(c_out // 16)
    if c_in <= 64:
        run = min(max(n_chunks * (c_out // 16 // nt) // 8192, 1), 16)
        return f"f32-runs-NT{nt}-run{run}"
    return f"f32-chunk-NT{nt}"


def pairs_x6_form_id(n_chunks, c_in, c_out):
    nt = local_nt(c_out)
    if c_in <= 128:
        run = min(max(n_chunks * (c_out // (16 * nt)) // 8192, 1), 16)
        return f"x6-runs-NT{nt}-KK{2 if c_in <= 64 else 4}-run{run}"
    return f"x6-chunk-NT{nt}"


def wgrad_x6_tile(c_in, c_out):
    a, b = c_in // 16, c_out // 16
    return pick_tile(a), (2 if b % 2 == 0 else 1)


def wgrad_pieces(total, K, c_in, c_out):
    """msp_wgrad_pieces."""
    if K < 1 or c_in < 16 or c_out < 16:
        return 1
    wa, wb = wgrad_x6_tile(c_in, c_out)
    n_ty = (c_in // (16 * wa)) * (c_out // (16 * wb))
    n = min(total // (K * 256), 4096 // (K * n_ty))
    if K == 1:
        n = min(n, 768)
    return max(n, 1)


def narrow_parts(V):
    """msp_conv_wgrad_narrow_parts."""
    return min(max(-(-max(V, 1) // 256), 1), 1024)


def split1_rows(c_out):
    """The smallest row count at which the shared-tile form of c_out runs unsplit."""
    t = 1
    while plan_x6(t * T, c_out)[3] != 1:
        t += 1
    return t * T


# ---------------------------------------------------------------- the GPU file's cases
def _case(entry, c_in, c_out, K, flip, kind, V, family, **kw):
    return dict(entry=entry, c_in=c_in, c_out=c_out, K=K, flip=flip, kind=kind, V=V, family=family, **kw)


def _families(entry, c_in, c_out, K, flip, **kw):
    """The non-integer families at FAMILY_ROWS on the ragged map and, for K = 27, the cloud."""
    out = []
    for V in FAMILY_ROWS:
        for kind in ("ragged", "cloud3") if K == 27 else ("ragged",):
            for fam in ("pieces-x", "pieces-w", "normal"):
                out.append(_case(entry, c_in, c_out, K, flip, kind, V, fam, **kw))
    return out


def tile_cases():
    """msp_conv_tile / msp_conv_tile_bn: the shared-tile form's five kernels and the per-wave form's six."""
    c = []
    E = "tile"
    c += [_case(E, 48, 48, 27, 0, "ragged", V, "integer") for V in ROWS]                 # x6d nt=3, every row edge
    c += [_case(E, 32, 16, 27, 2, "ragged", V, "integer", epi=True) for V in ROWS]       # x6r (16,32) + epilogue
    # x6d: one narrow and one wide shape per kernel
    for ci, co in ((16, 48), (48, 64), (224, 32), (128, 16)):
        c += _families(E, ci, co, 27, 0)
    for ci, co in ((64, 192), (64, 448), (64, 160), (64, 80), (448, 64)):
        c += [_case(E, ci, co, 27, 1, "ragged", 129, f) for f in ("integer", "pieces-x", "pieces-w")]
    c += [_case(E, 16, 448, 8, 0, "ragged", 4609, "integer")]                            # nt=4 nb=1 at 37 tiles
    c += [_case(E, 16, 448, 8, 2, "ragged", split1_rows(448), "integer")]                # a split of 1
    for K in (1, 8, 65, 128):                                                            # 65, 128: the second need word
        c += [_case(E, 48, 48, K, 0, "ragged", V, f) for V in (129, 1023) for f in ("integer", "pieces-x")]
    for flip in (1, 2, 3):
        c += [_case(E, 48, 96, 27, flip, "cloud3", 257, f) for f in ("integer", "pieces-w", "normal")]
    c += [_case(E, 48, 96, 27, 6, "cloud3", 257, "integer", image=True)]                 # flip bit 2
    for kind in ("centre", "hole"):                                                      # zero-fill split blocks
        c += [_case(E, 64, 160, 27, 0, kind, V, "integer") for V in (257, 1023)]
    c += [_case(E, 448, 224, 27, 0, "hole", 300, "integer")]                             # the deepest level's shape
    # x6r, (c_in, c_out): launch_x6r has NT in {1, 2} (16 or 32 columns) x NKK in {1, 2} (c_in up to 32 or 64);
    # (32, 16) is the ROWS sweep above, c_out = 64 exists only as the two-pass form from 10^5 rows
    for ci, co in ((16, 16), (16, 32), (64, 16), (64, 32), (48, 32)):
        c += _families(E, ci, co, 27, 2, epi=True)
        c += [_case(E, ci, co, 8, 1, "ragged", 129, "integer")]
    c += [_case(E, 16, 64, 2, 2, "full", 100000, "integer", epi=True)]                   # the two-pass form
    return c


def local_cases():
    c = []
    E = "local"
    c += [_case(E, 48, 48, 27, 2, "ragged", V, "integer", epi=True, shuffle=V % 2 == 0, wave_off=V % 3 != 0)
          for V in ROWS]
    for ci, co in ((16, 48), (64, 64)):
        c += _families(E, ci, co, 27, 2, shuffle=True, wave_off=True)
    for ci, co in ((48, 64), (192, 48), (64, 192)):
        c += [_case(E, ci, co, 27, 1, "cloud3", 1025, f, shuffle=False, wave_off=False, epi=True)
              for f in ("integer", "pieces-x", "pieces-w")]
    for K in (1, 8):
        c += [_case(E, 48, 64, K, 2, "ragged", 257, f, shuffle=True, wave_off=True) for f in ("integer", "pieces-x")]
    for wo in (True, False):
        c += [_case(E, 64, 48, 27, 1 + (not wo), "wide", 300, "integer", shuffle=wo, wave_off=wo)]
    c += [_case(E, 64, 64, 27, 2, "hole", 1023, "integer", shuffle=True, wave_off=True, epi=True)]
    return c


def nbr_cases():
    c = []
    E = "nbr"
    c += [_case(E, 48, 64, 27, 0, "ragged", V, "integer", perm=V % 2 == 1) for V in ROWS]
    for ci, co in ((16, 16), (64, 192)):
        c += _families(E, ci, co, 27, 2, perm=True)
    for K in (1, 128):
        c += [_case(E, 48, 64, K, 1, "ragged", 257, f, perm=False) for f in ("integer", "pieces-x", "pieces-w")]
    c += [_case(E, 64, 16, 27, 3, "hole", 1023, "integer", perm=True)]
    return c


PAIR_COUNTS = ((0, 1, 16, 0, 17, 33, 0), (17,), (0, 5), (1, 0, 0, 16, 0))


def pairs_cases():
    """msp_conv_pairs and msp_conv_pairs_x6 over one-offset-per-row maps: (entry, c_in, c_out, counts, family)."""
    c = []
    for E in ("pairs", "pairs_x6"):
        for ci, co in ((16, 16), (16, 80), (32, 32), (48, 48), (64, 64), (96, 32), (96, 80)):
            for fam in ("integer", "pieces-x", "pieces-w", "normal"):
                c.append(dict(entry=E, c_in=ci, c_out=co, counts=PAIR_COUNTS[0], family=fam))
        for counts in PAIR_COUNTS[1:]:
            c.append(dict(entry=E, c_in=32, c_out=48, counts=counts, family="integer"))
        # a run length above 1: c_out 80 (5 column groups of one), c_in 16, 3277 chunks
        c.append(dict(entry=E, c_in=16, c_out=80, counts=(0, 16 * 3000 + 1, 0, 16 * 276), family="integer"))
        c.append(dict(entry=E, c_in=64, c_out=32, counts=None, family="pieces-x"))       # a child map (K = 8)
    return c


WGRAD_COUNTS = (0, 1, 255, 0, 256, 257, 3, 0)


def wgrad_cases():
    """msp_conv_wgrad over pair lists: (c_in, c_out, kind, K, V, n_pieces, family); n_pieces 0 = the library's."""
    c = []
    for ci in (16, 32, 48, 64):
        for co in (16, 32):
            for npc, fam in ((1, "integer"), (4, "pieces-x"), (0, "pieces-w")):
                c.append(dict(entry="wgrad", c_in=ci, c_out=co, kind="counts", K=8, V=0, n_pieces=npc, family=fam))
    for npc in (1, 2, 3, 4, 5, 9, 0):
        c.append(dict(entry="wgrad", c_in=80, c_out=48, kind="counts", K=8, V=0, n_pieces=npc, family="integer"))
        c.append(dict(entry="wgrad", c_in=32, c_out=16, kind="cloud3", K=27, V=1025, n_pieces=npc, family="normal"))
    for V in ROWS:
        c.append(dict(entry="wgrad", c_in=32, c_out=32, kind="ragged", K=27, V=V, n_pieces=3, family="integer"))
    c.append(dict(entry="wgrad", c_in=16, c_out=16, kind="ragged", K=1, V=1025, n_pieces=5, family="pieces-x"))
    return c


WCHUNK_CAP = 448   # msp_wgrad_chunk_cap: distinct rows a tile of the chunk weight gradient stages


def wgrad_chunk_cases():
    """msp_conv_wgrad_chunk (+ msp_conv_wgrad_far): index "tile" = msp_wgrad_chunk_index over the tile rulebook
    and the tiles' row lists, "local" / "local-shuffled" = msp_local_chunk_index over the full tile-local
    rulebook; ranges 1, 0 = n_tiles, -1 = the library's own."""
    c = []
    E = "wgrad_chunk"
    rng_of = (1, 0, -1)
    for i, V in enumerate(ROWS):
        c.append(_case(E, 32, 32, 27, None, "ragged", V, "integer", index="tile", ranges=rng_of[i % 3]))
        c.append(_case(E, 32, 64, 27, None, "cloud3", V, "integer", index=("local", "local-shuffled")[i % 2],
                       ranges=rng_of[(i + 1) % 3]))
    for r in rng_of:
        c.append(_case(E, 64, 32, 27, None, "hole", 1023, "integer", index="tile", ranges=r))
        c.append(_case(E, 32, 64, 27, None, "wide", 300, "integer", index="tile", ranges=r))     # the far rules
    c.append(_case(E, 64, 64, 27, None, "wide", 300, "integer", index="tile", ranges=-1))
    for V in FAMILY_ROWS:
        for fam in ("pieces-x", "pieces-w", "normal"):
            c.append(_case(E, 32, 32, 27, None, "cloud3", V, fam, index="tile", ranges=-1))
            c.append(_case(E, 64, 96, 27, None, "cloud3", V, fam, index="local", ranges=0))
    for K in (1, 8):                                                     # not the 27-offset deal table
        c += [_case(E, 32, 32, K, None, "ragged", 257, f, index=ix, ranges=0)
              for f in ("integer", "pieces-x") for ix in ("tile", "local")]
    return c


def far_rules(m, cap=WCHUNK_CAP):
    """The number of rules whose input row lies past `cap` in its tile's sorted list of distinct rows."""
    n = 0
    for t in range(-(-m.shape[1] // T)):
        blk = m[:, t * T:(t + 1) * T]
        u = np.unique(blk[blk >= 0])
        n += int((np.searchsorted(u, blk[blk >= 0]) >= cap).sum())
    return n


NARROW_ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)
NARROW_SHAPES = tuple((ci, co) for ci in (1, 2, 3, 4) for co in (16, 32, 64))


def narrow_cases():
    """msp_conv_narrow_in / msp_conv_wgrad_narrow_in: (c_in, c_out, K, kind, V, family, n_parts); n_parts 0 = the
    library's, -1 = V + 3 (more parts than rows)."""
    c = []
    fams = ("integer", "pieces-x", "pieces-w")
    parts = (1, 2, 3, 0, -1)
    i = 0
    for ci, co in NARROW_SHAPES:
        for K in (1, 8, 27):
            V = NARROW_ROWS[i % len(NARROW_ROWS)]
            kind = "cloud3" if K == 27 and V > 1 and i % 2 else "ragged"
            c.append(dict(entry="narrow", c_in=ci, c_out=co, K=K, kind=kind, V=V, family=fams[i % 3],
                          n_parts=parts[i % 5]))
            i += 1
    for V in NARROW_ROWS:
        for npart in parts:
            c.append(dict(entry="narrow", c_in=3, c_out=32, K=27, kind="ragged", V=V, family="integer",
                          n_parts=npart))
    c.append(dict(entry="narrow", c_in=1, c_out=16, K=1, kind="centre", V=8192 * 256 + 5, family="integer",
                  n_parts=None))      # the forward's grid cap (forward only)
    c.append(dict(entry="narrow", c_in=1, c_out=16, K=1, kind="centre", V=262145, family="integer", n_parts=0,
                  wgrad_only=True))   # the weight gradient's parts cap
    return c


def case_map(c):
    """(map, n_in) of a case."""
    if "counts" in c:
        if c["counts"] is None:
            return make_map("cloud_down", 8, 700)
        return make_single_map(tuple(c["counts"]), sum(c["counts"]) + 5)
    if c["kind"] == "counts":
        return make_single_map(WGRAD_COUNTS, sum(WGRAD_COUNTS) + 5)
    return make_map(c["kind"], c["K"], c["V"])


def pairs_data(family, K, n_x, c_in, c_out, seed=0):
    """x [n_x][c_in] and wt [K][c_out][c_in] for the pair-list forward (one offset per output row, so an output
    element is a sum over the input channels only): the pieces-x selector has one input channel per (offset,
    output channel)."""
    rng = _rng(family, K, n_x, c_in, c_out, seed, 79)
    if family == "integer":
        return _ints(rng, (n_x, c_in)), _ints(rng, (K, c_out, c_in))
    if family == "pieces-x":
        wt = np.zeros((K, c_out, c_in), F32)
        for o in range(K):
            wt[o, np.arange(c_out), rng.integers(0, c_in, c_out)] = _pow2(rng, c_out)
        assert (wt != 0).sum(2).max() <= 1
        return _wide_values(rng, (n_x, c_in)), wt
    if family == "pieces-w":       # one non-zero input channel per x row: one term per output element
        x = np.zeros((n_x, c_in), F32)
        x[np.arange(n_x), rng.integers(0, c_in, n_x)] = _pow2(rng, n_x)
        return x, _wide_values(rng, (K, c_out, c_in))
    assert family == "normal"
    return rng.standard_normal((n_x, c_in)).astype(F32), (rng.standard_normal((K, c_out, c_in)) / c_in ** 0.5).astype(F32)


def case_id(c):
    keys = ("c_in", "c_out", "K", "flip", "kind", "V", "family", "n_parts", "n_pieces", "index", "ranges")
    s = "-".join(f"{k}{c[k]}" if k not in ("kind", "family", "index") else str(c[k]) for k in keys if c.get(k) is not None)
    if "counts" in c:
        s = c["entry"] + "-" + s
        s += "-child" if c["counts"] is None else f"-n{sum(c['counts'])}k{len(c['counts'])}"
    for flag in ("epi", "image", "shuffle", "wave_off", "perm", "wgrad_only"):
        if c.get(flag):
            s += "-" + flag
    return s
