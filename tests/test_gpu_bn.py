"""Every exported entry of csrc/msp_bn.hip against the fp64 restatements of tests/bn_ref.py, called through the C
ABI at the smallest shapes that reach each kernel form, grid edge and row edge.

Forms.  The entries choose a kernel from the channel count and the pointers' alignment; `reduce_form` and
`apply_form` below restate that dispatch, every test id names the form its case must take, and each test asserts
that the restatement agrees with its id.

Buffers.  Every array handed to the library is an interior view (`Dev`) of a larger device tensor: guard words
on both sides, outputs pre-filled with NaN.  After the call the guards must be intact, the inputs unchanged and
no NaN left where the entry must write.  "off4" cases start the view 4 bytes past a 16-byte boundary.

Inputs.  x is drawn from the stats a case passes in, x = mean + (zt - shift) / scale with |zt| in [0.05, 3], so
that no (leaky) ReLU decision sits on a rounding edge and no element has to be left out of a comparison;
tests/test_bn_ref.py asserts min |z| >= 1e-3 for every case listed in `relu_cases()`.  One channel in three has
test_batchnorm's regression geometry (mean / std = 1e3, mean_lo != 0).

Bounds are derived beside their use, from the arithmetic and not from the kernels' results.  Every test prints its
worst error / bound ratio (pytest -s).
"""
import functools
import math

import numpy as np
import pytest
import torch

import bn_ref as R
from sparseconvnet import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
G = 2048                      # guard words on either side of every view
GUARD = {F32: -7.0e37, F64: -7.0e300}
EPS, MOM = 1e-4, 0.9
LEAKS = [0.0, 0.333]


# ---------------------------------------------------------------- the dispatch, restated
def vec_ok(C):
    return C % 4 == 0 and C <= 1024


def reduce_form(C, aligned=True):
    """msp_bn_stats / msp_bn_bwd_stats / the reduction behind msp_add_bn_stats and msp_join_cols."""
    if vec_ok(C) and aligned:
        return "vector"
    return "scalar-narrow" if C <= 256 else "scalar-wide"


def apply_form(C, aligned=True):
    """msp_bn_apply / msp_bn_bwd_apply*."""
    return "vector" if vec_ok(C) and aligned else "scalar"


# (form of the reductions, C, elements the base pointers are off a 16-byte boundary)
FORMS = [("vector", 4, 0), ("vector", 32, 0), ("vector", 36, 0), ("vector", 260, 0), ("vector", 1024, 0),
         ("scalar-narrow", 1, 0), ("scalar-narrow", 3, 0), ("scalar-narrow", 6, 0),
         ("scalar-wide", 258, 0), ("scalar-wide", 1028, 0),
         ("scalar-narrow", 32, 1), ("scalar-wide", 260, 1)]


def _fid(f):
    return f"{f[0]}-C{f[1]}" + ("-off4" if f[2] else "")


def edge_rows(C, form):
    """The smallest V at each row edge of a form: R rows per block pass, U = 4 passes unrolled, rpb rows per
    partial block."""
    if form == "vector":
        Rr = 256 // (C // 4)
    elif form == "scalar-narrow":
        Rr = 256 // C
    else:
        Rr = 1
    vs = {0, 1, Rr - 1, Rr, Rr + 1, 4 * Rr - 1, 4 * Rr, 4 * Rr + 1, R.rows_per_block(C) + 1}
    return sorted(v for v in vs if v >= 0)


# (id, C, V): the partial cap with empty trailing blocks, and the grid-stride paths of rows_grid / ew_grid
BIG = [("vector-cap-empty-trailing", 1024, 16385), ("vector-cap-empty-trailing", 32, 262145),
       ("scalar-narrow-cap-empty-trailing", 6, 262145), ("scalar-wide-cap-empty-trailing", 258, 24577),
       ("vector-R1-rows-grid-stride", 1024, 4097), ("scalar-ew-grid-stride", 6, 174763),
       ("vector-R256-rows-grid-stride", 4, 4096 * 256 + 3)]


def _bid(b):
    return f"{b[0]}-C{b[1]}-V{b[2]}"


# (form of the apply, C, ca, elements dxb is off a 16-byte boundary)
SPLITS = [("vector-quad-stores", 64, 32, 0), ("vector-element-stores", 16, 6, 0), ("vector-element-stores", 8, 1, 0),
          ("vector-element-stores", 8, 7, 0), ("scalar-split", 64, 32, 1), ("scalar-split", 15, 6, 0),
          ("scalar-split", 258, 129, 0), ("scalar-split", 7, 1, 0)]
SPLIT_ROWS = [1, 2, 5, 64, 65, 257]

# (form, ca, cb, partial given, elements b is off a 16-byte boundary)
JOINS = [("mode3", 4, 4, True, 0), ("mode3", 32, 64, True, 0), ("mode3", 8, 252, True, 0),
         ("copy+vector", 6, 10, True, 0), ("copy+scalar-narrow", 3, 4, True, 0), ("copy-no-partial", 32, 64, False, 0),
         ("copy+vector", 32, 64, True, 1)]
ADDS = [("vector", 4, 0), ("vector", 36, 0), ("vector", 260, 0), ("vector", 1024, 0), ("add+scalar-narrow", 6, 0),
        ("add+scalar-wide", 258, 0), ("add+vector", 32, 1)]
CM_CASES = [(32, 0), (32, 1), (32, 257), (6, 0), (6, 1), (6, 257)]    # (C, P) of msp_bn_bwd_apply_cm
CM_ROWS = 100


# ---------------------------------------------------------------- inputs (numpy, fixed seeds; never modified)
def make_stats(C, weighted=True, seed=0):
    """stats[5][C] and the weight behind its scale.  Channels 0, 3, 6, ... are far from zero with a small
    deviation (mean 10, std 0.01); the signs of the weights are mixed."""
    rng = np.random.default_rng([C, seed, 17])
    far = np.arange(C) % 3 == 0
    mu = np.where(far, 10.0 + rng.uniform(-0.5, 0.5, C), rng.uniform(-2, 2, C))
    invstd = np.where(far, 100.0 * rng.uniform(0.8, 1.25, C), rng.uniform(0.5, 2, C)).astype(F32)
    weight = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
    bias = rng.uniform(-0.3, 0.3, C).astype(F32)
    hi = mu.astype(F32)
    lo = (mu - hi.astype(F64)).astype(F32)
    scale = (weight.astype(F64) * invstd.astype(F64)).astype(F32) if weighted else invstd
    return np.stack([hi, lo, invstd, scale, bias]), (weight if weighted else None)


def _make_case(C, V, weighted=True, seed=0):
    stats, weight = make_stats(C, weighted, seed)
    rng = np.random.default_rng([C, V, seed, 29])
    zt = rng.uniform(0.05, 3.0, (V, C)) * rng.choice([-1.0, 1.0], (V, C))
    mean = stats[0].astype(F64) + stats[1].astype(F64)
    x = (mean + (zt - stats[4].astype(F64)) / stats[3].astype(F64)).astype(F32)
    g = rng.standard_normal((V, C)).astype(F32)
    addend = rng.standard_normal((V, C)).astype(F32)
    return dict(C=C, V=V, stats=stats, weight=weight, x=x, g=g, addend=addend)


_cached_case = functools.lru_cache(maxsize=None)(_make_case)


def case(C, V, weighted=True, seed=0):
    """The arrays of one case, shared read-only by the tests (the few multi-megabyte ones are rebuilt)."""
    return (_cached_case if V * C <= 1 << 17 else _make_case)(C, V, weighted, seed)


def relu_cases():
    """Every (C, V, weighted) whose x meets a (leaky) ReLU decision in a test below."""
    out = set()
    for form, C, _ in FORMS:
        for V in edge_rows(C, form):
            out.add((C, V, True))
            out.add((C, V, False))
    for _, C, V in BIG:
        out.add((C, V, True))
    for _, C, _, _ in SPLITS:
        for V in SPLIT_ROWS:
            out.add((C, V, True))
            out.add((C, V, False))
    for C, _ in CM_CASES:
        out.add((C, CM_ROWS, True))
        out.add((C, CM_ROWS, False))
    return sorted(out)


# ---------------------------------------------------------------- the buffer harness
class Dev:
    """[data | n_out NaNs] as an interior view of a larger device tensor with G guard words on both sides; `off`
    moves the view that many elements past a 16-byte boundary."""

    def __init__(self, data=None, n_out=0, dtype=F32, off=0):
        if data is not None:
            data = np.ascontiguousarray(data, dtype).reshape(-1)
        self.n_in = 0 if data is None else data.size
        self.n, self.off, self.dtype = self.n_in + n_out, off, dtype
        tdt = torch.float32 if dtype == F32 else torch.float64
        self.big = torch.full((G + off + self.n + G,), GUARD[dtype], dtype=tdt, device=DEV)
        self.lo = G + off
        item = self.big.element_size()
        self.ptr = self.big.data_ptr() + self.lo * item
        assert self.big.data_ptr() % 16 == 0 and self.ptr % 16 == (off * item) % 16
        self.src = data
        if self.n_in:
            self.big[self.lo:self.lo + self.n_in].copy_(torch.from_numpy(data))
        if n_out:
            self.big[self.lo + self.n_in:self.lo + self.n].fill_(float("nan"))

    def check(self, written=None, what=""):
        """Guards intact, the input part unchanged, no NaN in the first `written` (default all) output elements;
        returns the view's contents."""
        big = self.big.cpu().numpy()
        guard = np.array(GUARD[self.dtype], self.dtype)
        assert (big[:self.lo] == guard).all(), f"{what}: words before the buffer overwritten"
        assert (big[self.lo + self.n:] == guard).all(), f"{what}: words after the buffer overwritten"
        got = big[self.lo:self.lo + self.n]
        if self.n_in:
            assert np.array_equal(got[:self.n_in].view(np.uint8), self.src.view(np.uint8)), f"{what}: input modified"
        w = self.n - self.n_in if written is None else written
        assert not np.isnan(got[self.n_in:self.n_in + w]).any(), f"{what}: output left unwritten"
        return got


def run(name, *args):
    _lib.call(name, *args, _lib.stream())
    torch.cuda.synchronize()


def refused(name, *args):
    """A host-side argument check: non-zero return, msp_last_error names the entry, nothing launched."""
    lib = _lib.load()
    rc = getattr(lib, name)(*args, _lib.stream())
    msg = lib.msp_last_error()
    torch.cuda.synchronize()
    assert rc != 0 and name.encode() in msg, (name, rc, msg)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v)).astype(F32)).astype(F64)


def ratio(err, bound):
    """Worst err / bound; where the bound is 0 the error must be 0."""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    assert np.isfinite(err).all()
    zero = bound == 0
    assert (err[zero] == 0).all(), "error where the bound is exactly zero"
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


class Worst:
    """The worst ratio of a test, printed with its id."""

    def __init__(self, label):
        self.label, self.worst = label, {}

    def add(self, r, what, key=""):
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        assert r < 1.0, f"{self.label} {what}: error / bound = {r:.3f}"

    def done(self):
        print(f"{self.label}: worst error / bound", ", ".join(f"{k} {v:.3g}".strip() for k, v in self.worst.items()))


def check_partials(buf, sums, C, w, what):
    """A [P][2][C] partial buffer against the reference sums: fp64 reordering of at most 2^18 terms per channel
    stays far inside 1e-12 of the sum of the terms' magnitudes -- for the P slots added on the host, and for each
    slot over its own rows [p per, min(V, (p + 1) per))."""
    P = sums.P
    got = buf.check(written=P * 2 * C, what=what)[:P * 2 * C].reshape(P, 2, C)
    w.add(ratio(np.abs(got.sum(0) - sums.total), 1e-12 * sums.mag), what + " totals")
    w.add(ratio(np.abs(got - sums.slots), 1e-12 * sums.slot_mag), what + " slots")
    return got


def partial_dev(C, P, off=0):
    return Dev(n_out=(P + 1) * 2 * C, dtype=F64, off=off)


# ---------------------------------------------------------------- msp_bn_partials
def test_partials_match_restatement():
    lib = _lib.load()
    for C in [1, 3, 4, 32, 63, 64, 65, 256, 260, 512, 513, 1024, 1025, 4096]:
        rpb = R.rows_per_block(C)
        for V in [0, 1, rpb - 1, rpb, rpb + 1, 7 * rpb + 3, 1024 * rpb, 1024 * rpb + 1, 1 << 31, (1 << 40) + 5]:
            assert lib.msp_bn_partials(V, C) == R.partials(V, C), (V, C)


# ---------------------------------------------------------------- the statistics passes
def _fwd_stats(C, V, off, w, what):
    c = case(C, V)
    P = R.partials(V, C)
    x, part = Dev(c["x"], off=off), partial_dev(C, P)
    run("msp_bn_stats", x.ptr, V, C, part.ptr)
    x.check(what=what)
    check_partials(part, R.fwd_sums(c["x"]), C, w, what)


def _bwd_stats(C, V, off, leak, w, what):
    c = case(C, V)
    P = R.partials(V, C)
    x, g, st, part = Dev(c["x"], off=off), Dev(c["g"], off=off), Dev(c["stats"]), partial_dev(C, P)
    run("msp_bn_bwd_stats", x.ptr, g.ptr, V, C, st.ptr, float(leak), part.ptr)
    for b in (x, g, st):
        b.check(what=what)
    check_partials(part, R.bwd_sums(c["x"], c["g"], c["stats"], leak), C, w, what)


@pytest.mark.parametrize("form,C,off", FORMS, ids=map(_fid, FORMS))
def test_stats(form, C, off):
    assert reduce_form(C, off == 0) == form
    w = Worst(f"msp_bn_stats {_fid((form, C, off))}")
    for V in edge_rows(C, form):
        _fwd_stats(C, V, off, w, f"V={V}")
    w.done()


@pytest.mark.parametrize("leak", LEAKS)
@pytest.mark.parametrize("form,C,off", FORMS, ids=map(_fid, FORMS))
def test_bwd_stats(form, C, off, leak):
    assert reduce_form(C, off == 0) == form
    w = Worst(f"msp_bn_bwd_stats {_fid((form, C, off))} leak {leak}")
    for V in edge_rows(C, form):
        _bwd_stats(C, V, off, leak, w, f"V={V}")
    w.done()


@pytest.mark.parametrize("name,C,V", BIG, ids=map(_bid, BIG))
def test_stats_cap_and_grid(name, C, V):
    """Blocks past the last row must still write zeros (the finalize adds all P slots of an uninitialised
    buffer): here they would stay NaN."""
    assert name.split("-")[0] == reduce_form(C).split("-")[0]
    w = Worst(f"msp_bn_stats {_bid((name, C, V))}")
    _fwd_stats(C, V, 0, w, f"V={V}")
    w.done()


@pytest.mark.parametrize("name,C,V", BIG[:4], ids=map(_bid, BIG[:4]))
def test_bwd_stats_cap(name, C, V):
    assert name.startswith(reduce_form(C))
    w = Worst(f"msp_bn_bwd_stats {_bid((name, C, V))}")
    _bwd_stats(C, V, 0, 0.333, w, f"V={V}")
    w.done()


# ---------------------------------------------------------------- residual add and channel join with statistics
def _stats_of(out_dev, V, C):
    """msp_bn_stats on an output view as it lies (same alignment, so the same form)."""
    P = R.partials(V, C)
    part = partial_dev(C, P)
    run("msp_bn_stats", out_dev.ptr, V, C, part.ptr)
    return part.check(written=P * 2 * C)[:P * 2 * C]


@pytest.mark.parametrize("form,C,off", ADDS, ids=map(_fid, ADDS))
def test_add_bn_stats(form, C, off):
    """sum bit-equal to a + b; its partials bit-equal to msp_bn_stats on that sum and inside the fp64 bound."""
    assert form == ("" if not off and vec_ok(C) else "add+") + reduce_form(C)   # the sum itself is aligned
    w = Worst(f"msp_add_bn_stats {_fid((form, C, off))}")
    for V in edge_rows(C, reduce_form(C)):
        c = case(C, V)
        P = R.partials(V, C)
        a, b, s, part = Dev(c["x"]), Dev(c["addend"], off=off), Dev(n_out=V * C), partial_dev(C, P)
        run("msp_add_bn_stats", a.ptr, b.ptr, V, C, s.ptr, part.ptr)
        a.check(), b.check()
        ref = R.add(c["x"], c["addend"])
        got = s.check(what=f"V={V}").reshape(V, C)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"V={V}: sum"
        gp = check_partials(part, R.fwd_sums(ref), C, w, f"V={V}")
        assert np.array_equal(gp.reshape(-1).view(np.uint64), _stats_of(s, V, C).view(np.uint64)), \
            f"V={V}: partials differ from msp_bn_stats on the sum"
    w.done()


def _jid(j):
    return f"{j[0]}-{j[1]}+{j[2]}" + ("-b-off4" if j[4] else "")


@pytest.mark.parametrize("form,ca,cb,with_partial,off", JOINS, ids=map(_jid, JOINS))
def test_join_cols(form, ca, cb, with_partial, off):
    """out bit-equal to [a | b]; the partials bit-equal to msp_bn_stats on out and inside the fp64 bound."""
    C = ca + cb
    if with_partial:
        mode3 = ca % 4 == 0 and cb % 4 == 0 and vec_ok(C) and not off
        assert form == ("mode3" if mode3 else "copy+" + reduce_form(C))
    w = Worst(f"msp_join_cols {_jid((form, ca, cb, with_partial, off))}")
    for V in edge_rows(C, reduce_form(C)):
        c = case(C, V)
        av, bv = R.split_cols(c["x"], ca)
        P = R.partials(V, C)
        a, b, out = Dev(av), Dev(bv, off=off), Dev(n_out=V * C)
        part = partial_dev(C, P) if with_partial else None
        run("msp_join_cols", a.ptr, ca, b.ptr, cb, V, out.ptr, part.ptr if part else None)
        a.check(), b.check()
        got = out.check(what=f"V={V}").reshape(V, C)
        assert np.array_equal(got.view(np.uint32), R.join_cols(av, bv).view(np.uint32)), f"V={V}: join"
        if part:
            gp = check_partials(part, R.fwd_sums(c["x"]), C, w, f"V={V}")
            assert np.array_equal(gp.reshape(-1).view(np.uint64), _stats_of(out, V, C).view(np.uint64)), \
                f"V={V}: partials differ from msp_bn_stats on the join"
    w.done()


@pytest.mark.parametrize("which", ["both", "a-null", "b-null"])
@pytest.mark.parametrize("form,ca,cb,off", [("quads", 4, 4, 0), ("quads", 32, 64, 0), ("elements", 6, 10, 0),
                                            ("elements", 3, 4, 0), ("elements", 32, 64, 1)],
                         ids=["quads-4+4", "quads-32+64", "elements-6+10", "elements-3+4", "elements-32+64-in-off4"])
def test_split_cols(form, ca, cb, off, which):
    assert form == ("quads" if ca % 4 == 0 and cb % 4 == 0 and not off else "elements")
    C = ca + cb
    for V in [0, 1, 5, 257]:
        c = case(C, V)
        ra, rb = R.split_cols(c["x"], ca)
        xin = Dev(c["x"], off=off)
        a = Dev(n_out=V * ca) if which != "a-null" else None
        b = Dev(n_out=V * cb) if which != "b-null" else None
        run("msp_split_cols", xin.ptr, V, ca, cb, a.ptr if a else None, b.ptr if b else None)
        xin.check()
        for d, ref in ((a, ra), (b, rb)):
            if d is not None:
                assert np.array_equal(d.check(what=f"V={V}").view(np.uint32), ref.reshape(-1).view(np.uint32)), V


# ---------------------------------------------------------------- finalize
def _slot_rows(V, P):
    v0, v1 = R.slot_bounds(V, P) if P > 0 else (np.zeros(0), np.zeros(0))
    n = (v1 - v0).astype(F64)
    return n if V > 0 else np.ones(P)       # V = 0: the slots hold anything finite, the guard must ignore them


def finalize_partials(P, V, C, seed=0):
    """[P][2][C] random doubles of mixed sign whose totals give a variance of 0.5 .. 4; channel 0 holds x == 3.0
    on every row (sums exact in any order: var == 0 exactly), channel 1 sums that leave S1 / V - mu^2 slightly
    negative (about -1e-11, far beyond fp64 reordering: the clamp)."""
    rng = np.random.default_rng([P, C, seed, 41])
    n = _slot_rows(V, P)[:, None]
    p = np.zeros((P, 2, C))
    if P == 0:
        return p
    p[:, 0] = rng.normal(0.3, 2.0, (P, C)) * n
    p[:, 1] = rng.normal(0.0, 5.0, (P, C)) * n
    nv = max(float(n.sum()), 1.0)
    mu = p[:, 0].sum(0) / nv
    p[:, 1] += n * (rng.uniform(0.5, 4.0, C) + mu * mu - p[:, 1].sum(0) / nv)
    if V > 0:
        p[:, 0, 0], p[:, 1, 0] = 3.0 * n[:, 0], 9.0 * n[:, 0]
        if C > 1:
            a = 0.7
            p[:, 0, 1], p[:, 1, 1] = a * n[:, 0], a * a * (1 - 2.0 ** -35) * n[:, 0]
    return p


def check_finalize(got, ref, tot, mag, V, train, w, what):
    """The float32 outputs of a finalize against the reference over the same partials (totals by math.fsum)."""
    st, rm, rv = got
    mu, var = ref["stats64"][0], ref["var"]
    if train and V > 0:
        # The kernel adds the P <= 1024 slots strided over 256 threads and then in a tree: a different fp64 order
        # from fsum's exact total, each partial sum bounded by sum |slot|.  d_mu is that reordering bound of the
        # mean, d_var the same for S1 / V plus the two propagated terms of mu^2 and the expression's own
        # roundings (one each for the quotient, the square and the difference).
        d_mu = 2.0 ** -50 * mag[0] / V
        d_var = 2.0 ** -50 * mag[1] / V + 2 * np.abs(mu) * d_mu + d_mu ** 2 + 2.0 ** -51 * (np.abs(tot[1]) / V + mu * mu)
    else:
        d_mu = d_var = np.zeros_like(mu)
    # mean pair: hi = f32(mu'), lo = f32(mu' - hi) with |mu' - hi| <= 2^-24 |mu'|, so lo's rounding is at most
    # 2^-48 |mu'|; 2^-46 |mu| covers it, d_mu is the kernel's own mu' against mu.
    pair = st[0].astype(F64) + st[1].astype(F64)
    w.add(ratio(np.abs(pair - mu), 2.0 ** -46 * np.abs(mu) + d_mu + 1e-300), what + " mean pair")
    # invstd = (var + eps)^-1/2: d invstd / invstd = -0.5 d_var / (var + eps); then one rounding to float32, which
    # can land on the neighbouring float when the fp64 values straddle a tie: one ulp.
    rel = 0.5 * d_var / (var + EPS)
    for row, name in ((2, "invstd"), (3, "scale")):
        r64 = ref["stats64"][row]
        w.add(ratio(np.abs(st[row].astype(F64) - ref["stats"][row].astype(F64)), ulp32(r64) + np.abs(r64) * rel),
              f"{what} {name}")
    assert np.array_equal(st[4], ref["stats"][4]), what + " shift"
    if train:
        # running = momentum * old + (1 - momentum) * (mu | var V / (V - 1)), rounded once to float32
        unb = V / (V - 1.0) if V > 1 else 1.0
        w.add(ratio(np.abs(rm.astype(F64) - ref["rmean"].astype(F64)), ulp32(ref["rmean64"]) + (1 - MOM) * d_mu),
              what + " running mean")
        w.add(ratio(np.abs(rv.astype(F64) - ref["rvar"].astype(F64)),
                    ulp32(ref["rvar64"]) + (1 - MOM) * unb * d_var), what + " running var")
    else:
        assert np.array_equal(rm, ref["rmean"]) and np.array_equal(rv, ref["rvar"]), what + " running stats"
        assert np.array_equal(st[0], ref["rmean"]) and not st[1].any(), what + " eval mean"


def _running(C):
    return np.linspace(-1, 1, C).astype(F32), np.linspace(0.5, 2, C).astype(F32)


def _finalize(layout, P, V, C, train, affine, w, what, null_partial=False):
    p = finalize_partials(P, V, C)
    stats0, weight = make_stats(C, affine, seed=3)
    bias = stats0[4] if affine else None
    rm0, rv0 = _running(C)
    data = p if layout == "rm" else np.transpose(p, (1, 2, 0))
    part = Dev(data, n_out=2 * C, dtype=F64)
    rm, rv, st = Dev(rm0), Dev(rv0), Dev(n_out=5 * C)
    wd, bd = (Dev(weight), Dev(bias)) if affine else (None, None)
    pp = None if null_partial else part.ptr
    wb = (wd.ptr if affine else None, bd.ptr if affine else None)
    if layout == "rm":
        assert R.partials(V, C) == P
        run("msp_bn_finalize", pp, V, C, EPS, MOM, int(train), rm.ptr, rv.ptr, *wb, st.ptr)
    else:
        run("msp_bn_finalize_cm", pp, P, V, C, EPS, MOM, int(train), rm.ptr, rv.ptr, *wb, st.ptr)
    part.check(written=0, what=what)
    # running statistics are updated in place: read them without the input comparison
    rm.src = rv.src = None
    rm.n_in = rv.n_in = 0
    tot, mag = R.partial_totals(p, "rm") if P > 0 else (np.zeros((2, C)), np.zeros((2, C)))
    ref = R.finalize(tot, V, C, EPS, MOM, train, rm0, rv0, weight, bias)
    got = (st.check(what=what).reshape(5, C), rm.check(written=0), rv.check(written=0))
    check_finalize(got, ref, tot, mag, V, train, w, what)
    if train and V > 0:
        assert got[0][2, 0] == F32(1.0 / math.sqrt(EPS)), what + ": var == 0 exactly (x == 3.0)"
        if C > 1 and P > 0:
            assert tot[1, 1] / V - (tot[0, 1] / V) ** 2 < 0 and got[0][2, 1] == F32(1.0 / math.sqrt(EPS)), \
                what + ": negative variance clamped"


# P = 1, 255, 256, 257, 1024 through (V, C): C = 5 has 256 rows per block; V = 0, 1, 2 give P = 1, V = 1000 P = 4
FIN_RM = [(0, 5), (1, 5), (2, 5), (1000, 5), (1000, 1024), (255 * 256, 5), (256 * 256, 5), (257 * 256, 5),
          (1024 * 256, 5), (1 << 30, 3)]


@pytest.mark.parametrize("V,C", FIN_RM, ids=[f"V{v}-C{c}-P{R.partials(v, c)}" for v, c in FIN_RM])
def test_finalize(V, C):
    P = R.partials(V, C)
    w = Worst(f"msp_bn_finalize V={V} C={C} P={P}")
    for train, affine in [(1, True), (1, False), (0, True), (0, False)]:
        _finalize("rm", P, V, C, train, affine, w, f"train={train} affine={affine}")
    w.done()


@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 1000])
def test_finalize_cm(P):
    w = Worst(f"msp_bn_finalize_cm P={P}")
    for V in [0, 1, 2, 1000]:
        for train, affine in [(1, True), (1, False), (0, True)]:
            _finalize("cm", P, V, 7, train, affine, w, f"V={V} train={train} affine={affine}")
    _finalize("cm", P, 1000 if P else 2, 7, 0, True, w, "eval, partial NULL", null_partial=True)
    w.done()


# ---------------------------------------------------------------- apply
def _apply(C, V, off, leak, w, what):
    c = case(C, V)
    x, st, y = Dev(c["x"], off=off), Dev(c["stats"]), Dev(n_out=V * C, off=off)
    run("msp_bn_apply", x.ptr, V, C, st.ptr, float(leak), y.ptr)
    x.check(), st.check()
    got = y.check(what=what).reshape(V, C)
    ref, mag = R.apply(c["x"], c["stats"], leak)
    # z = xc * scale + shift with xc exact in the reference: two roundings (product, sum) of at most 2^-24 of
    # |xc scale| and of |z| <= |xc scale| + |shift|, or one when fused; z * leak adds 2^-24 |y| <= 2^-24 |z|
    # and scales the rest by leak < 1: under 3 * 2^-24 (|xc scale| + |shift|) < 2^-22 (...).
    w.add(ratio(np.abs(got.astype(F64) - ref), 2.0 ** -22 * mag), what)


@pytest.mark.parametrize("leak", LEAKS)
@pytest.mark.parametrize("form,C,off", FORMS, ids=[f"{apply_form(f[1], not f[2])}-C{f[1]}" + ("-off4" if f[2] else "")
                                                   for f in FORMS])
def test_apply(form, C, off, leak):
    w = Worst(f"msp_bn_apply {apply_form(C, off == 0)}-C{C}{'-off4' if off else ''} leak {leak}")
    for V in edge_rows(C, form):
        _apply(C, V, off, leak, w, f"V={V}")
    w.done()


@pytest.mark.parametrize("name,C,V", BIG[4:], ids=map(_bid, BIG[4:]))
def test_apply_grid_stride(name, C, V):
    assert name.startswith(apply_form(C))
    w = Worst(f"msp_bn_apply {_bid((name, C, V))}")
    _apply(C, V, 0, 0.333, w, f"V={V}")
    w.done()


# ---------------------------------------------------------------- backward apply
# Roundings of bn_bwd_apply4_kernel's f (and of the scalar kernel's body) on the way from the reference's float32
# dz and xc to d, train mode: ws = fl(w invstd), mdz = fl(S0 / V), mdzx = fl(S1 / V), xh = fl(xc invstd),
# fl(xh mdzx), fl(dz - mdz), fl(. - .), fl(ws .): 8, each at most 2^-24 of an intermediate no larger than
# |dz| + |S0 / V| + |xhat S1 / V|, times |w invstd|.  Eval mode: ws and the product, 2 -- a worst case that single
# elements among thousands come close to, so the eval ratios sit just under 1 and the train ratios near 1/2.
ROUNDINGS = {1: 8, 0: 2}
# (train, addend, weight, dweight / dbias)
BWD_VARIANTS = [(1, False, True, True), (1, True, True, True), (0, False, True, True), (0, True, False, False),
                (1, True, False, False)]


def bwd_partials(c, leak, P):
    """The reference's own per-slot sums as the partial buffer the entry reads, and their totals by fsum."""
    sums = R.bwd_sums(c["x"], c["g"], c["stats"], leak, P)
    tot, _ = R.partial_totals(sums.slots, "rm")
    return sums.slots, tot


def check_dx(got, ref, mag, train, with_addend, w, what):
    bound = ROUNDINGS[train] * 2.0 ** -24 * mag
    if with_addend:
        bound = bound + ulp32(ref)          # one more float32 add
    w.add(ratio(np.abs(got.astype(F64) - ref), bound), what, "train" if train else "eval")


def check_totals(part, n_slots, tot, dw, db, C, what):
    """The [2][C] tail holds the totals (fp64 reordering of the slots: 1e-12 of their magnitudes), dbias and
    dweight are the totals rounded to float32."""
    buf = part.check(what=what)
    tail = buf[n_slots:].reshape(2, C)
    mag = np.abs(buf[:n_slots]).reshape(-1, 2, C).sum(0) if part.layout == "rm" else \
        np.abs(buf[:n_slots]).reshape(2, C, -1).sum(-1)
    assert ratio(np.abs(tail - tot), 1e-12 * mag) < 1.0, what + " totals"
    if db is not None:
        assert np.array_equal(db.check(what=what), tot[0].astype(F32)), what + " dbias"
        assert np.array_equal(dw.check(what=what), tot[1].astype(F32)), what + " dweight"


def _bwd_apply(C, V, off, leak, variant, w, what, split=None, cm=None):
    """One call of msp_bn_bwd_apply (no addend), _add, _split (split = (ca, dxb off)) or _cm (cm = P)."""
    train, with_add, weighted, with_grads = variant
    c = case(C, V, weighted)
    if cm is None:
        P = R.partials(V, C)
        slots, tot = bwd_partials(c, leak, P)
        part = Dev(slots, n_out=2 * C, dtype=F64)
        part.layout = "rm"
    else:
        P = cm
        rng = np.random.default_rng([C, P, 53])
        slots = rng.standard_normal((2, C, P)) * V / max(P, 1)
        tot = R.partial_totals(slots, "cm")[0] if P else np.zeros((2, C))
        part = Dev(slots, n_out=2 * C, dtype=F64)
        part.layout = "cm"
    x, g, st = Dev(c["x"], off=off), Dev(c["g"], off=off), Dev(c["stats"])
    wd = Dev(c["weight"]) if weighted else None
    ad = Dev(c["addend"], off=off) if with_add else None
    dw, db = (Dev(n_out=C), Dev(n_out=C)) if with_grads else (None, None)
    opt = lambda d: d.ptr if d is not None else None
    head = (x.ptr, g.ptr, V, C, part.ptr)
    if split is not None:
        ca, boff = split
        dxa, dxb = Dev(n_out=V * ca, off=off), Dev(n_out=V * (C - ca), off=boff)
        run("msp_bn_bwd_apply_split", *head, st.ptr, opt(wd), float(leak), train, opt(ad), ca, dxa.ptr, dxb.ptr,
            opt(dw), opt(db))
        outs = [dxa, dxb]
    else:
        dx = Dev(n_out=V * C, off=off)
        outs = [dx]
        if cm is not None:
            run("msp_bn_bwd_apply_cm", *head, P, st.ptr, opt(wd), float(leak), train, opt(ad), dx.ptr, opt(dw),
                opt(db))
        elif with_add:
            run("msp_bn_bwd_apply_add", *head, st.ptr, opt(wd), float(leak), train, opt(ad), dx.ptr, opt(dw), opt(db))
        else:
            run("msp_bn_bwd_apply", *head, st.ptr, opt(wd), float(leak), train, dx.ptr, opt(dw), opt(db))
    for b in (x, g, st, wd, ad):
        if b is not None:
            b.check(what=what)
    check_totals(part, slots.size, tot, dw, db, C, what)
    ref, mag = R.bwd_apply(c["x"], c["g"], tot, c["stats"], c["weight"], leak, train,
                           c["addend"] if with_add else None, None if split is None else split[0])
    if split is None:
        ref, mag = [ref], [mag]
    for o, r, m in zip(outs, ref, mag):
        check_dx(o.check(what=what).reshape(r.shape), r, m, train, with_add, w, what)


@pytest.mark.parametrize("form,C,off", FORMS, ids=[f"{apply_form(f[1], not f[2])}-C{f[1]}" + ("-off4" if f[2] else "")
                                                   for f in FORMS])
def test_bwd_apply(form, C, off):
    """msp_bn_bwd_apply and msp_bn_bwd_apply_add: train and eval, addend NULL and given, weight NULL,
    dweight / dbias NULL."""
    w = Worst(f"msp_bn_bwd_apply[_add] {apply_form(C, off == 0)}-C{C}{'-off4' if off else ''}")
    for V in edge_rows(C, form):
        for i, variant in enumerate(BWD_VARIANTS):
            _bwd_apply(C, V, off, LEAKS[i % 2], variant, w, f"V={V} {variant}")
    w.done()


@pytest.mark.parametrize("name,C,V", BIG[4:], ids=map(_bid, BIG[4:]))
def test_bwd_apply_grid_stride(name, C, V):
    assert name.startswith(apply_form(C))
    w = Worst(f"msp_bn_bwd_apply_add {_bid((name, C, V))}")
    _bwd_apply(C, V, 0, 0.333, (1, True, True, True), w, f"V={V}")
    w.done()


def _sid(s):
    return f"{s[0]}-C{s[1]}-ca{s[2]}" + ("-dxb-off4" if s[3] else "")


@pytest.mark.parametrize("form,C,ca,boff", SPLITS, ids=map(_sid, SPLITS))
def test_bwd_apply_split(form, C, ca, boff):
    """msp_bn_bwd_apply_split: the columns [0, ca) in dxa [V][ca], the rest in dxb [V][C - ca]."""
    if vec_ok(C) and (ca % 4 != 0 or not boff):
        assert form == ("vector-quad-stores" if ca % 4 == 0 else "vector-element-stores")
    else:
        assert form == "scalar-split"
    w = Worst(f"msp_bn_bwd_apply_split {_sid((form, C, ca, boff))}")
    for V in SPLIT_ROWS:
        for i, variant in enumerate(BWD_VARIANTS):
            _bwd_apply(C, V, 0, LEAKS[i % 2], variant, w, f"V={V} {variant}", split=(ca, boff))
    w.done()


@pytest.mark.parametrize("C,P", CM_CASES, ids=[f"{apply_form(c)}-C{c}-P{p}" for c, p in CM_CASES])
def test_bwd_apply_cm(C, P):
    """msp_bn_bwd_apply_cm: the totals of a channel-major [2][C][P] buffer (mixed-sign doubles), then the apply."""
    w = Worst(f"msp_bn_bwd_apply_cm {apply_form(C)}-C{C} P={P}")
    for i, variant in enumerate(BWD_VARIANTS):
        _bwd_apply(C, CM_ROWS, 0, LEAKS[i % 2], variant, w, f"{variant}", cm=P)
    w.done()


# ---------------------------------------------------------------- argument checks (host side, nothing launched)
def test_argument_checks():
    C, V = 8, 4
    c = case(C, V)
    x, g, st = Dev(c["x"]), Dev(c["g"]), Dev(c["stats"])
    out = Dev(n_out=V * C)
    part = partial_dev(4097, 1)
    for bad in (0, 4097):
        refused("msp_bn_stats", x.ptr, V, bad, part.ptr)
        refused("msp_bn_bwd_stats", x.ptr, g.ptr, V, bad, st.ptr, 0.0, part.ptr)
    dxa, dxb = Dev(n_out=V * C), Dev(n_out=V * C)
    for ca in (0, C):
        refused("msp_bn_bwd_apply_split", x.ptr, g.ptr, V, C, part.ptr, st.ptr, None, 0.0, 1, None, ca, dxa.ptr,
                dxb.ptr, None, None)
    refused("msp_bn_bwd_apply_add", x.ptr, g.ptr, V, C, part.ptr, st.ptr, None, 0.0, 1, out.ptr, out.ptr, None, None)
    refused("msp_join_cols", x.ptr, 4, g.ptr, 4, V, x.ptr, None)
    refused("msp_add_bn_stats", x.ptr, g.ptr, V, C, x.ptr, part.ptr)
    for b in (x, g, st):
        b.check()
    for b in (out, dxa, dxb, part):          # nothing ran: every output is still NaN, every guard intact
        assert np.isnan(b.check(written=0)).all()
