"""The BatchNorm restatements of tests/bn_ref.py checked themselves (CPU): chained and held against
oracle/scn_oracle.py in double (autograd's own adjoint, not the oracle's hand-written one), the partition against
hand-computed values, and the inputs of tests/test_gpu_bn.py against the condition its comparisons rest on -- no
(leaky) ReLU decision within 1e-3 of zero -- so that a later edit of a generator cannot quietly remove it."""
import numpy as np
import pytest
import torch

import bn_ref as R
import test_gpu_bn as G
from oracle import scn_oracle as O

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("V", [1, 2, 257])
@pytest.mark.parametrize("leak", [0.0, 0.333])
@pytest.mark.parametrize("train", [True, False])
def test_chain_matches_oracle(train, leak, V, monkeypatch):
    """sums -> finalize -> apply, then backward sums -> backward apply, all in fp64 (fp64 arrays: nothing in the
    reference rounds), against BatchNormLeakyReLU in double under autograd: forward, dx, dweight, dbias and the
    running statistics within 1e-12 of each tensor's scale.  dx is a difference of terms that nearly cancel at
    V = 2 (xhat = +-1: what is left is of the order eps / var of the terms), so its scale is that of its terms,
    |w invstd| (|dz| + |mean dz| + |xhat mean(dz xhat)|), which both sides round at 1e-16.  The float32 outputs of
    finalize are the roundings of the fp64 ones."""
    monkeypatch.setattr(O, "LEAN", False)
    C, eps, mom = 5, 1e-4, 0.9
    rng = np.random.default_rng([V, int(train), int(leak * 1000)])
    x = rng.normal(1.5, 3.0, (V, C))
    gy = rng.standard_normal((V, C))
    w, b = rng.uniform(0.5, 1.5, C) * np.array([1, -1, 1, -1, 1.0]), rng.uniform(-0.2, 0.3, C)
    rm0, rv0 = np.linspace(-1, 1, C), np.linspace(0.5, 2, C)

    bo = O.BatchNormLeakyReLU(C, eps=eps, momentum=mom, leakiness=leak).double()
    with torch.no_grad():
        bo.weight.copy_(torch.from_numpy(w))
        bo.bias.copy_(torch.from_numpy(b))
        bo.running_mean.copy_(torch.from_numpy(rm0))
        bo.running_var.copy_(torch.from_numpy(rv0))
    bo.train(train)
    xo = torch.from_numpy(x).requires_grad_(True)
    yo = bo(O.OTensor(xo, None, 8)).features
    (yo * torch.from_numpy(gy)).sum().backward()

    sums = R.fwd_sums(x)
    direct = np.stack([x.sum(0), (x * x).sum(0)])
    assert np.allclose(sums.total, direct, rtol=1e-13, atol=0) and sums.slots.shape == (R.partials(V, C), 2, C)
    fin = R.finalize(sums.total, V, C, eps, mom, train, rm0, rv0, w, b)
    st = fin["stats64"]
    y, _ = R.apply(x, st, leak)
    bs = R.bwd_sums(x, gy, st, leak)
    dx, dx_terms = R.bwd_apply(x, gy, bs.total, st, w, leak, train)

    def close(got, ref, what, scale=0.0):
        ref = ref.detach().numpy()
        assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), scale, 1e-300), what

    close(y, yo, "forward")
    close(dx, xo.grad, "dx", dx_terms.max())
    close(bs.total[1], bo.weight.grad, "dweight")
    close(bs.total[0], bo.bias.grad, "dbias")
    close(fin["rmean64"], bo.running_mean, "running mean")
    close(fin["rvar64"], bo.running_var, "running var")
    # the float32 outputs: the mean as a pair, the rest rounded once
    f = fin["stats"]
    assert f.dtype == F32 and fin["rmean"].dtype == F32
    assert np.all(np.abs(f[0].astype(F64) + f[1].astype(F64) - st[0]) <= 2.0 ** -46 * np.abs(st[0]))
    assert np.array_equal(f[2:], st[2:].astype(F32))
    assert np.array_equal(fin["rmean"], fin["rmean64"].astype(F32))
    assert np.array_equal(fin["rvar"], fin["rvar64"].astype(F32))


def test_finalize_edges():
    """V = 0 gives mean = var = 0 whatever the sums hold; a negative variance is clamped; NULL weight / bias mean
    1 and 0; V = 1 leaves the variance biased."""
    tot = np.array([[3.0, 0.7], [9.0, 0.7 * 0.7 * (1 - 2.0 ** -35)]])
    rm0, rv0 = np.zeros(2, F32), np.ones(2, F32)
    f = R.finalize(tot * 5, 0, 2, 1e-4, 0.9, 1, rm0, rv0, None, None)
    assert not f["stats64"][0].any() and not f["var"].any() and np.array_equal(f["stats"][3], f["stats"][2])
    assert not f["stats"][4].any() and np.array_equal(f["rvar64"], [0.9, 0.9])
    f = R.finalize(tot, 1, 2, 1e-4, 0.9, 1, rm0, rv0, None, None)
    assert tot[1, 1] - tot[0, 1] ** 2 < 0 and not f["var"].any()
    assert np.array_equal(f["stats"][2], np.full(2, 100, F32))
    f = R.finalize(np.array([[2.0], [10.0]]), 2, 1, 0.0, 0.5, 1, rm0[:1], rv0[:1], None, None)
    assert f["var"][0] == 4.0 and f["rvar64"][0] == 0.5 + 0.5 * 8.0 and f["rmean64"][0] == 0.5


def test_float32_steps_are_the_kernels():
    """With float32 arrays the centring is two rounded float32 subtractions and dz one rounded float32 product."""
    c = G.case(6, 9)
    x, st, g = c["x"], c["stats"], c["g"]
    xc = R.centred(x, st)
    assert xc.dtype == F32
    assert np.array_equal(xc, ((x - st[0]).astype(F32) - st[1]).astype(F32))
    dz = R.dz_of(x, g, st, 0.333)
    neg = R.z_of(x, st) <= 0
    assert dz.dtype == F32 and neg.any() and (~neg).any()
    assert np.array_equal(dz[neg], g[neg] * F32(0.333)) and np.array_equal(dz[~neg], g[~neg])
    # dropping mean_lo moves z of a far channel by far more than the apply's rounding bound
    y, mag = R.apply(x, st, 0.0)
    st0 = st.copy()
    st0[1] = 0
    y0, _ = R.apply(x, st0, 0.0)
    assert st[1].all() and (np.abs(y - y0) > 2.0 ** -22 * mag).any()


# ---------------------------------------------------------------- the partition
RPB = {1: 256, 64: 128, 65: 120, 512: 16, 513: 16, 1024: 16, 1025: 256, 4096: 256}


@pytest.mark.parametrize("C", sorted(RPB))
def test_partials_at_the_clamp_edges(C):
    rpb = RPB[C]
    assert R.rows_per_block(C) == rpb
    got = [R.partials(V, C) for V in (0, 1, rpb, rpb + 1, 1024 * rpb, 1024 * rpb + 1)]
    assert got == [1, 1, 1, 2, 1024, 1024]


def test_partials_hand_values():
    assert R.partials(1000, 64) == 8 and R.partials(1000, 1024) == 63 and R.partials(2500, 32) == 10
    assert R.partials(16385, 1024) == 1024 and R.partials(300000, 65) == 1024 and R.partials(257, 5) == 2
    v0, v1 = R.slot_bounds(16385, 1024)            # 17 rows a slot: 963 full, one of 14, the rest empty
    assert v1[962] - v0[962] == 17 and v1[963] - v0[963] == 14 and not (v1[964:] - v0[964:]).any()
    v0, v1 = R.slot_bounds(262145, 1024)
    assert np.count_nonzero(v1 > v0) == 1021 and v1.max() == 262145
    v0, v1 = R.slot_bounds(0, 1)
    assert v0[0] == v1[0] == 0


def test_slot_sums_partition_the_total():
    x = G.case(3, 1025)["x"]
    s = R.fwd_sums(x)
    assert s.P == 5
    v0, v1 = R.slot_bounds(1025, 5)
    for p in range(5):
        assert np.allclose(s.slots[p, 0], x[v0[p]:v1[p]].astype(F64).sum(0), rtol=1e-14, atol=0)
        assert np.allclose(s.slot_mag[p, 1], (x[v0[p]:v1[p]].astype(F64) ** 2).sum(0), rtol=1e-14, atol=0)


# ---------------------------------------------------------------- the GPU tests' inputs
def test_gpu_inputs_keep_relu_decisions_off_the_edge():
    """min |z_ref| >= 1e-3 (about 10^4 float32 ulps of an O(1) value) over every element of every input the GPU
    tests draw, so those tests compare every element."""
    cases = G.relu_cases()
    assert len(cases) > 100
    worst = np.inf
    for C, V, weighted in cases:
        c = G.case(C, V, weighted)
        assert c["x"].shape == (V, C) and c["x"].dtype == F32 and c["stats"].dtype == F32
        if V:
            worst = min(worst, np.abs(R.z_of(c["x"], c["stats"])).min())
    print(f"min |z_ref| over {len(cases)} cases: {worst:.4f}")
    assert worst >= 1e-3


def test_gpu_cases_reach_the_edges_they_name():
    """The finalize cases reach P = 1, 255, 256, 257 and 1024; the cap cases leave trailing slots empty; the
    grid-stride cases exceed 4096 blocks of their kernels; the clamp channel's variance is negative."""
    assert {R.partials(v, c) for v, c in G.FIN_RM} >= {1, 255, 256, 257, 1024}
    for name, C, V in G.BIG:
        if "cap-empty-trailing" in name:
            v0, v1 = R.slot_bounds(V, R.partials(V, C))
            assert R.partials(V, C) == 1024 and V > 1024 * R.rows_per_block(C) and not (v1[-1] - v0[-1])
        elif "rows-grid" in name:
            assert -(-V // (256 // (C // 4))) > 4096
        else:
            assert -(-V * C // 256) > 4096 and -(-(V - 1) * C // 256) <= 4096
    for P, V in [(1, 1), (4, 1000), (1024, 1 << 30)]:
        p = G.finalize_partials(P, V, 5)
        tot, _ = R.partial_totals(p, "rm")
        assert tot[0, 0] == 3.0 * V and tot[1, 0] == 9.0 * V
        assert tot[1, 1] / V - (tot[0, 1] / V) ** 2 < -1e-12
        assert (p[:, :, 2:] < 0).any() or P == 1
        var = tot[1, 2:] / V - (tot[0, 2:] / V) ** 2
        assert (var > 0.4).all() and (var < 4.1).all()
