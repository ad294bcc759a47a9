"""Plain numpy restatements of the BatchNorm family of csrc/msp_bn.hip, one function per exported entry (CPU only;
nothing of the package's ops is imported).  Each takes the arrays the entry takes and returns what it must write,
in fp64 unless the entry's contract is bit-exact.

The functions are dtype-generic on purpose.  With the float32 arrays the entries take they reproduce the kernels'
own float32 steps (the two rounded subtractions of the mean pair, the float32 dz = g * leak) and do everything
else in fp64; with fp64 arrays nothing rounds, which is how tests/test_bn_ref.py holds them against
oracle/scn_oracle.py to 1e-12.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MAX_PARTS = 1024     # kMaxParts
STAT_ROWS = 5        # stats[5][C]: mean_hi, mean_lo, invstd, scale, shift


# ---------------------------------------------------------------- the partition
def rows_per_block(C):
    rpb = 8 * (1024 // C) if 0 < C <= 1024 else 256
    return min(max(rpb, 16), 256)


def partials(V, C):
    """msp_bn_partials: the number of slots of a [P][2][C] partial buffer."""
    rpb = rows_per_block(C)
    return min(max(-(-V // rpb), 1), MAX_PARTS)


def slot_bounds(V, P):
    """Rows [v0[p], v1[p]) of slot p: per = ceil(V / P) rows each, trailing slots empty."""
    per = -(-V // P)
    v0 = np.minimum(np.arange(P, dtype=np.int64) * per, V)
    return v0, np.minimum(v0 + per, V)


class Sums:
    """Per-channel sums of two term arrays [V][C]: total [2][C], slots [P][2][C], and the sums of magnitudes."""

    def __init__(self, t0, t1, P):
        V, C = t0.shape
        self.P = P
        self.slots = np.zeros((P, 2, C), F64)
        self.slot_mag = np.zeros((P, 2, C), F64)
        v0, v1 = slot_bounds(V, P)
        live = v1 > v0
        if live.any():
            for k, t in enumerate((t0, t1)):
                self.slots[live, k] = np.add.reduceat(t, v0[live], axis=0)
                self.slot_mag[live, k] = np.add.reduceat(np.abs(t), v0[live], axis=0)
        self.total = self.slots.sum(0)
        self.mag = self.slot_mag.sum(0)


def fwd_sums(x, P=None):
    """msp_bn_stats: (sum x, sum x^2) per channel."""
    xd = x.astype(F64)
    return Sums(xd, xd * xd, partials(*x.shape) if P is None else P)


# ---------------------------------------------------------------- per-element pieces
def centred(x, stats):
    """(x - mean_hi) - mean_lo: two separately rounded subtractions in the arrays' own precision."""
    return (x - stats[0]) - stats[1]


def z_of(x, stats):
    return centred(x, stats).astype(F64) * stats[3].astype(F64) + stats[4].astype(F64)


def dz_of(x, g, stats, leak):
    """The gradient through the (leaky) ReLU, in g's precision (float32 for the entries: one rounded product)."""
    return np.where(z_of(x, stats) > 0, g, g * g.dtype.type(leak)).astype(g.dtype)


def xhat_of(x, stats):
    return centred(x, stats).astype(F64) * stats[2].astype(F64)


def bwd_sums(x, g, stats, leak, P=None):
    """msp_bn_bwd_stats: (sum dz, sum dz * xhat) per channel."""
    dz = dz_of(x, g, stats, leak).astype(F64)
    return Sums(dz, dz * xhat_of(x, stats), partials(*x.shape) if P is None else P)


# ---------------------------------------------------------------- finalize
def partial_totals(partial, layout):
    """[2][C] exact-rounded totals (math.fsum) of partial [P][2][C] ('rm') or [2][C][P] ('cm'), and sum |slot|."""
    p = partial if layout == "cm" else np.transpose(partial, (1, 2, 0))
    C = p.shape[1]
    tot = np.array([[math.fsum(p[k, c].tolist()) for c in range(C)] for k in range(2)], F64).reshape(2, C)
    return tot, np.abs(p).sum(-1).reshape(2, C)


def finalize(totals, V, C, eps, momentum, train, rmean, rvar, weight, bias):
    """msp_bn_finalize / msp_bn_finalize_cm from the per-channel totals [2][C].  Returns the float32 outputs
    (stats [5][C], rmean, rvar) and the unrounded fp64 values they were rounded from (stats64 with the whole mean
    in row 0, rmean64, rvar64, var)."""
    rm64, rv64 = rmean.astype(F64), rvar.astype(F64)
    if train:
        if V > 0:
            mu = totals[0] / V
            var = np.maximum(totals[1] / V - mu * mu, 0.0)
        else:
            mu, var = np.zeros(C), np.zeros(C)
        unb = var * V / (V - 1) if V > 1 else var
        rm64 = momentum * rm64 + (1.0 - momentum) * mu
        rv64 = momentum * rv64 + (1.0 - momentum) * unb
    else:
        mu, var = rm64, rv64
    invstd = 1.0 / np.sqrt(var + eps)
    w = np.ones(C) if weight is None else weight.astype(F64)
    b = np.zeros(C) if bias is None else bias.astype(F64)
    hi = mu.astype(F32)
    stats = np.stack([hi, (mu - hi.astype(F64)).astype(F32), invstd.astype(F32), (w * invstd).astype(F32),
                      b.astype(F32)])
    stats64 = np.stack([mu, np.zeros(C), invstd, w * invstd, b])
    return dict(stats=stats, rmean=rm64.astype(F32), rvar=rv64.astype(F32), stats64=stats64, rmean64=rm64,
                rvar64=rv64, var=var)


# ---------------------------------------------------------------- apply and its backward
def leaky(z, leak):
    return np.where(z > 0, z, z * leak)


def apply(x, stats, leak):
    """msp_bn_apply: y = leaky(z), and the magnitude |xc * scale| + |shift| its rounding bound is stated in."""
    xc = centred(x, stats).astype(F64)
    t = xc * stats[3].astype(F64)
    sh = stats[4].astype(F64)
    return leaky(t + sh, F64(x.dtype.type(leak))), np.abs(t) + np.abs(sh)


def bwd_apply(x, g, totals, stats, weight, leak, train, addend=None, ca=None):
    """msp_bn_bwd_apply / _add / _split / _cm from the per-channel totals [2][C] of msp_bn_bwd_stats.  Returns d
    (a pair split at column ca when ca is given) and the magnitude |w invstd| (|dz| + |S0/V| + |xhat S1/V|)."""
    V, C = x.shape
    dz = dz_of(x, g, stats, leak).astype(F64)
    w = np.ones(C) if weight is None else weight.astype(F64)
    wis = w * stats[2].astype(F64)
    if train:
        m0 = totals[0] / V if V > 0 else np.zeros(C)
        m1 = totals[1] / V if V > 0 else np.zeros(C)
        xh = xhat_of(x, stats)
        d = wis * (dz - m0 - xh * m1)
        mag = np.abs(wis) * (np.abs(dz) + np.abs(m0) + np.abs(xh * m1))
    else:
        d = wis * dz
        mag = np.abs(wis) * np.abs(dz)
    if addend is not None:
        d = d + addend.astype(F64)
    if ca is not None:
        return (d[:, :ca], d[:, ca:]), (mag[:, :ca], mag[:, ca:])
    return d, mag


# ---------------------------------------------------------------- join / split / add (bit-exact)
def join_cols(a, b):
    return np.concatenate([a, b], 1)


def split_cols(x, ca):
    return x[:, :ca].copy(), x[:, ca:].copy()


def add(a, b):
    """One float32 add per element (msp_add_bn_stats's sum)."""
    return a + b
