"""The builders and references of tests/conv_ref.py checked themselves (CPU): the rulebooks against the contract
checkers, the references against oracle/scn_oracle.py on a small real cloud (which ties the flip and layout
conventions to the oracle and not to the kernels), the exactness / one-term property of every case
tests/test_gpu_conv_forms.py lists, and the sensitivity of the comparison the GPU file uses."""
import numpy as np
import pytest
import torch

import conv_ref as R
import metadata_ref as MR
from oracle import scn_oracle as O

MAPS = [("centre", 27, 257), ("full", 8, 129), ("ragged", 27, 1), ("ragged", 27, 129), ("ragged", 128, 257),
        ("ragged", 1, 1025), ("hole", 27, 1023), ("hole", 8, 300), ("wide", 27, 300), ("cloud3", 27, 1),
        ("cloud3", 27, 1025), ("cloud_down", 8, 700)]


@pytest.mark.parametrize("kind,K,V", MAPS)
def test_rulebooks_meet_their_contracts(kind, K, V):
    m, n_in = R.make_map(kind, K, V)
    V = m.shape[1]
    tl = R.tile_rulebook(m)
    info = MR.check_tile_rulebook(m, V, 128, tl["tile_start"], tl["chunk_off"], tl["chunk_src"], tl["chunk_row"])
    assert info["n_chunks"] == tl["n_chunks"]
    if K <= 32:
        for shuffle in (None, 3):
            for wo in (True, False):
                loc = R.local_rulebook(m, shuffle=shuffle, wave_off=wo)
                if wo and K <= 27:
                    R.check_local_rulebook(m, loc, V)
                else:
                    assert loc["wave_off"] is None
                    R.check_local_rulebook(m, dict(loc, wave_off=R.local_rulebook(m, shuffle=shuffle)["wave_off"]), V)
    rb = R.pair_rulebook(m)
    assert rb["total"] == int((m >= 0).sum()) and rb["chunk_start"][-1] == rb["n_chunks"]
    assert np.array_equal(np.diff(rb["chunk_start"]), -(-np.diff(rb["off_start"]) // 16))
    perm, mp = R.dense_order(m)
    assert sorted(perm.tolist()) == list(range(V)) and np.array_equal(mp, m[:, perm])


def test_map_edges_present():
    """The edges the GPU cases rely on: (tile, offset) groups of 0, 1, 15, 16, 17, 127 and 128 entries, an empty
    tile in the middle and at the end, tiles of exactly 383 / 384 distinct rows."""
    m, _ = R.make_map("ragged", 27, 1025)
    cnt = {int((m[o, t * 128:(t + 1) * 128] >= 0).sum()) for t in range(8) for o in range(27)}
    assert cnt >= set(R.RAGGED)
    h, _ = R.make_map("hole", 27, 1023)
    per_tile = [(h[:, t * 128:(t + 1) * 128] >= 0).sum() for t in range(8)]
    assert per_tile[4] == 0 and per_tile[7] == 0 and min(per_tile[:4]) > 0
    s, _ = R.make_single_map((0, 1, 16, 0, 17, 33, 0), 80)
    assert [(s[o] >= 0).sum() for o in range(7)] == [0, 1, 16, 0, 17, 33, 0]
    w, _ = R.make_map("wide", 27, 300)      # asserts its 383 / 384 distinct-row tiles itself
    assert R.far_rules(w) > 0 and R.far_rules(w, 10 ** 6) == 0    # a tile past the chunk weight gradient's 448
    # msp_local_chunk_index takes no far rules; the ragged maps of the "tile" index have some of their own
    assert all(R.far_rules(R.case_map(c)[0]) == 0 for c in R.wgrad_chunk_cases() if c["index"] != "tile")
    assert R.far_rules(R.make_map("ragged", 27, 1025)[0]) > 0 and R.far_rules(R.make_map("cloud3", 27, 1025)[0]) == 0


def _oracle_tensor(coords, feats, size):
    t = O.InputLayer(3, size, mode=4)([torch.from_numpy(coords), torch.from_numpy(feats)])
    return t, t.metadata.levels[size].coords


def test_references_match_oracle():
    """fwd / wgrad / pairs on a small real cloud against the oracle's SubmanifoldConvolution, Convolution and
    Deconvolution, forward and backward, in fp64."""
    c, size = R.cloud(700, 5)
    rng = np.random.default_rng(0)
    ci, co = 5, 7
    # the oracle's rows are in raster order, the reference's in Morton order
    t, ocoords = _oracle_tensor(c, rng.standard_normal((len(c), ci)), size)
    to_o = MR.row_map(c, ocoords, size)                    # reference row -> oracle row
    x = t.features.numpy()[to_o]                            # the same features, reference row order
    # --- submanifold, 3^3
    m = MR.subm_map(c, size, 3)
    conv = O.SubmanifoldConvolution(3, ci, co, 3, False).double()
    xo = t.features.clone().requires_grad_(True)
    yo = conv(O.OTensor(xo, t.metadata, size)).features
    g = torch.from_numpy(rng.standard_normal(tuple(yo.shape)))
    yo.backward(g)
    W = conv.weight.detach().numpy()[:, 0]                 # [K][c_in][c_out]
    gy = g.numpy()[to_o]
    assert np.allclose(R.fwd(x, W, m, 2), yo.detach().numpy()[to_o], rtol=0, atol=1e-12)
    assert np.allclose(R.fwd(x, W.transpose(0, 2, 1), m, 0), yo.detach().numpy()[to_o], rtol=0, atol=1e-12)
    # backward-data: the forward weights with offsets mirrored (flip bit 0), channels swapped
    dx = R.fwd(gy, W, m, 1)                                # w given [K][c_out'][c_in'] = [K][c_in][c_out]
    assert np.allclose(dx, xo.grad.numpy()[to_o], rtol=0, atol=1e-12)
    assert np.allclose(R.fwd(gy, W.transpose(0, 2, 1), m, 3), xo.grad.numpy()[to_o], rtol=0, atol=1e-12)
    assert np.allclose(R.wgrad(x, gy, m), conv.weight.grad.numpy()[:, 0], rtol=0, atol=1e-12)
    # --- strided convolution 2 / 2 and its deconvolution
    dn = MR.down_map(c, 1)
    down = dn["down"]
    sc = O.Convolution(3, ci, co, 2, 2, False).double()
    xo = t.features.clone().requires_grad_(True)
    tc = sc(O.OTensor(xo, t.metadata, size))
    c_to_o = MR.row_map(dn["coarse"], t.metadata.levels[size // 2].coords, size // 2)
    g = torch.from_numpy(rng.standard_normal(tuple(tc.features.shape)))
    tc.features.backward(g)
    Ws = sc.weight.detach().numpy()[:, 0]
    gyc = g.numpy()[c_to_o]
    assert np.allclose(R.fwd(x, Ws, down, 2), tc.features.detach().numpy()[c_to_o], rtol=0, atol=1e-12)
    assert np.allclose(R.wgrad(x, gyc, down), sc.weight.grad.numpy()[:, 0], rtol=0, atol=1e-12)
    rb = R.pair_rulebook(down, swap=True)                  # coarse row -> fine row, one pair per fine row
    dxs = R.pairs(gyc, Ws, rb["pair_in"], rb["pair_out"], rb["off_start"], len(c))   # wt [K][c_in][c_out] here
    assert np.allclose(dxs, xo.grad.numpy()[to_o], rtol=0, atol=1e-12)
    dc = O.Deconvolution(3, co, ci, 2, 2, False).double()
    xc = tc.features.detach().clone().requires_grad_(True)
    yf = dc(O.OTensor(xc, t.metadata, size // 2)).features
    g = torch.from_numpy(rng.standard_normal(tuple(yf.shape)))
    yf.backward(g)
    Wd = dc.weight.detach().numpy()[:, 0]                  # [K][c_in = co][c_out = ci]
    xcr = xc.detach().numpy()[c_to_o]
    assert np.allclose(R.pairs(xcr, Wd.transpose(0, 2, 1), rb["pair_in"], rb["pair_out"], rb["off_start"], len(c)),
                       yf.detach().numpy()[to_o], rtol=0, atol=1e-12)
    # deconvolution backward-data gathers over the child map; its weight gradient runs over the swapped pairs
    assert np.allclose(R.fwd(g.numpy()[to_o], Wd, down, 0), xc.grad.numpy()[c_to_o], rtol=0, atol=1e-12)
    dwd = R.wgrad(g.numpy()[to_o], xcr, down).transpose(0, 2, 1)
    assert np.allclose(dwd, dc.weight.grad.numpy()[:, 0], rtol=0, atol=1e-12)


def test_tile_rulebook_gives_the_maps_sum():
    m, n_in = R.make_map("ragged", 8, 129)
    x, w = R.fwd_data("integer", m, n_in, 16, 16, 1)
    assert np.array_equal(R.fwd_tiles(x, w, R.tile_rulebook(m), 129, 1), R.fwd(x, w, m, 1))


def test_epi_partial_by_hand():
    out = np.arange(130 * 2, dtype=np.float32).reshape(130, 2)
    p = R.epi_partial(out)
    assert p.shape == (2, 2, 2)
    assert p[0, 1, 0] == out[:128, 1].astype(np.float64).sum() and p[1, 0, 1] == float(out[128, 0]) ** 2 + float(out[129, 0]) ** 2


def _forward_cases():
    return R.tile_cases() + R.local_cases() + R.nbr_cases()


@pytest.mark.parametrize("entry", ["forward", "pairs", "wgrad", "wgrad_chunk", "narrow"])
def test_gpu_cases_hold_their_family_property(entry):
    """Every exact-family case the GPU file lists builds (the builders assert sum |x||w| < 2^24 for the integer
    family and the one-term property for the pieces families); the widest forward's bound by hand."""
    assert 27 * 448 * 9 < 1 << 24 and 262145 * 9 < 1 << 24
    n = 0
    if entry == "forward":
        for c in _forward_cases():
            if c["family"] in R.EXACT and c["V"] * c["c_in"] * c["c_out"] * c["K"] <= 1 << 31:
                m, n_in = R.case_map(c)
                R.fwd_data(c["family"], m, n_in, c["c_in"], c["c_out"], c["flip"] & 3)
                n += 1
    elif entry == "pairs":
        for c in R.pairs_cases():
            m, n_in = R.case_map(c)
            x, wt = R.pairs_data(c["family"], m.shape[0], max(n_in, m.shape[1]), c["c_in"], c["c_out"])
            if c["family"] == "integer":
                assert c["c_in"] * 9 < 1 << 24
            n += 1
    elif entry in ("wgrad", "wgrad_chunk"):
        for c in R.wgrad_cases() if entry == "wgrad" else R.wgrad_chunk_cases():
            if c["family"] in R.EXACT:
                m, n_in = R.case_map(c)
                R.wgrad_data(c["family"], m, n_in, c["c_in"], c["c_out"])
                n += 1
    else:
        for c in R.narrow_cases():
            m, n_in = R.case_map(c)
            if not c.get("wgrad_only") and m.shape[1] < 1 << 20:
                R.fwd_data(c["family"], m, n_in, c["c_in"], c["c_out"], 2)
            if c["n_parts"] is not None:
                R.wgrad_data(c["family"], m, n_in, c["c_in"], c["c_out"])
            n += 1
    assert n > 10


def test_case_ids_are_distinct():
    for cases in (R.tile_cases(), R.local_cases(), R.nbr_cases(), R.pairs_cases(), R.wgrad_cases(), R.wgrad_chunk_cases(),
                  R.narrow_cases()):
        got = [R.case_id(c) for c in cases]
        assert len(set(got)) == len(got), [g for g in got if got.count(g) > 1]


def test_restated_plan_regimes():
    """1023 rows (8 tiles) and 1025 (9 tiles) straddle plan_x6's two split regimes; nt=4 nb=1 needs 256 blocks."""
    assert R.plan_x6(1023, 48) == (3, 2, 1, 16) and R.plan_x6(1025, 48) == (3, 2, 1, 8)
    assert R.plan_x6(4609, 448) == (4, 1, 7, 4) and R.plan_x6(4608, 448)[:2] == (4, 2)
    assert R.plan_x6(R.split1_rows(448), 448)[3] == 1 and R.plan_x6(R.split1_rows(448) - 128, 448)[3] > 1
    assert R.use_x6r(100000, 16, 64) and not R.use_x6r(99999, 16, 64)
    forms = {R.tile_form_id(c["V"], c["c_in"], c["c_out"]).split("-split")[0].rsplit("-ny", 1)[0] for c in R.tile_cases()}
    assert {"x6d-nt3-nb2", "x6d-nt4-nb2", "x6d-nt2-nb2", "x6d-nt1-nb2", "x6d-nt4-nb1"} <= forms, forms


def test_comparison_is_sensitive():
    """The GPU file's comparison reports a dropped rule, two swapped chunk_row entries and one ulp."""
    m, n_in = R.make_map("ragged", 8, 129)
    x, w = R.fwd_data("integer", m, n_in, 16, 16, 0)
    ref = R.fwd(x, w, m, 0)
    R.compare_exact(ref.astype(np.float32), ref)
    m2 = m.copy()
    o, r = (int(v[0]) for v in np.nonzero(m >= 0))
    m2[o, r] = -1
    assert np.abs(x[m[o, r]]).max() > 0
    with pytest.raises(AssertionError, match="differ"):
        R.compare_exact(R.fwd(x, w, m2, 0).astype(np.float32), ref, "dropped rule")
    tl = R.tile_rulebook(m)
    rows = tl["chunk_row"].copy()
    c0 = int(np.nonzero(tl["chunk_off"] == 3)[0][0]) * 16     # a chunk with at least two entries
    assert rows[c0] < 128 and rows[c0 + 1] < 128
    rows[c0], rows[c0 + 1] = rows[c0 + 1], rows[c0]
    with pytest.raises(AssertionError, match="differ"):
        R.compare_exact(R.fwd_tiles(x, w, dict(tl, chunk_row=rows), 129, 0).astype(np.float32), ref, "swapped rows")
    xn, wn = R.fwd_data("pieces-x", m, n_in, 16, 16, 0)
    refn = R.fwd(xn, wn, m, 0)
    got = refn.astype(np.float32)
    i = tuple(int(v[0]) for v in np.nonzero(got))
    got[i] = np.nextafter(got[i], np.float32(np.inf))
    with pytest.raises(AssertionError, match="1 of"):
        R.compare_exact(got, refn, "one ulp")
    nan = np.full((2, 2), np.nan, np.float32)
    R.compare_exact(nan, nan.astype(np.float64))
    with pytest.raises(AssertionError):
        R.compare_exact(np.zeros((2, 2), np.float32), nan.astype(np.float64))
