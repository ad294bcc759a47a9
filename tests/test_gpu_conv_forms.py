"""Every convolution entry of the C ABI on small rulebooks built on the CPU (tests/conv_ref.py), at the tile,
chunk, row-group and split edges of each kernel form, against fp64 references taken straight from the map.

Forms.  conv_ref restates the dispatch (use_x6r, plan_x6, launch_x6r's NT / NKK, local_nt, pick_tile and the run
length of the pair forms, wgrad_x6_tile); every test id carries the form its case must take, and each test asserts
the restatement against what the library exports (msp_conv_tile_form, and msp_conv_tile_workspace_size, whose
value round256(weights) + split * n_rows * c_out * 4 reveals the split).  A disagreement fails the case.

Buffers.  Every array goes to the library as an interior view (`Buf`) of a larger device tensor with guard bytes
on both sides; outputs are pre-filled with NaN; a workspace has exactly the bytes its size query returns, so the
guard behind it is its canary.  After the call the guards are intact, the inputs unchanged and no NaN is left in
the n_rows x c_out output (for the pair forms: rows no pair names are still NaN).  Every case runs twice and the
two outputs are bitwise equal.

Checks.  The integer, pieces-x and pieces-w families are exact (conv_ref asserts why), so the comparison is
equality with the reference rounded to fp32.  The normal family keeps the bars tests/test_gpu_ops.py states for
each form: x6d / x6r <= max(3 x a plain fp32 evaluation's error, 1e-7) and < 1e-6 of the output scale, conv_nbr
the same with 2 x, conv_local and the chunk weight gradient < 1e-6, the pair forms (f32 and x6) and the pair-list
weight gradient 1e-5.  Each prints its
worst error and bound (pytest -s).
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as R
from sparseconvnet import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
G = 4096            # guard bytes on either side of every view
GB = 0xA5


# ---------------------------------------------------------------- the buffer harness
class Buf:
    """[G guard bytes | payload | G guard bytes] in one device tensor.  data: an input (checked unchanged);
    out_floats: that many float32 NaNs; out_doubles: float64 NaNs; ws: that many bytes of workspace."""

    def __init__(self, data=None, out_floats=0, out_doubles=0, ws=0):
        if data is not None:
            self.src = np.ascontiguousarray(data).reshape(-1).view(np.uint8).copy()
            self.n = self.src.size
        else:
            self.src = None
            self.n = out_floats * 4 + out_doubles * 8 + ws
        self.big = torch.full((G + self.n + G,), GB, dtype=torch.uint8, device=DEV)
        self.ptr = self.big.data_ptr() + G
        assert self.ptr % 256 == 0
        body = self.big[G:G + self.n]
        if self.src is not None and self.n:
            body.copy_(torch.from_numpy(self.src))
        elif out_floats:
            body.view(torch.float32).fill_(float("nan"))
        elif out_doubles:
            body.view(torch.float64).fill_(float("nan"))

    def check(self, what=""):
        assert bool((self.big[:G] == GB).all()), f"{what}: bytes before the buffer overwritten"
        assert bool((self.big[G + self.n:] == GB).all()), f"{what}: bytes after the buffer overwritten"
        if self.src is not None and self.n:
            assert np.array_equal(self.big[G:G + self.n].cpu().numpy(), self.src), f"{what}: input modified"

    def array(self, dtype, shape):
        return self.big[G:G + self.n].cpu().numpy().view(dtype).reshape(shape)


def call(name, *args):
    _lib.call(name, *args, _lib.stream())
    torch.cuda.synchronize()


def fails(name, text, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args, _lib.stream())
    torch.cuda.synchronize()
    msg = lib.msp_last_error().decode(errors="replace")
    assert rc != 0 and text in msg, (name, rc, msg)


def q(name, *args):
    return int(getattr(_lib.load(), name)(*args))


def twice(run, inputs, what):
    """run() -> dict of output arrays, two times on fresh output buffers; the two runs are bitwise equal and every
    input, guard and canary is intact after each."""
    a = run()
    for b in inputs:
        b.check(what)
    b2 = run()
    for b in inputs:
        b.check(what)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b2[k].view(np.uint8)), f"{what}: {k} differs between two runs"
    return a


def verdict(c, got, ref, what, mult, plain=None):
    if c["family"] in R.EXACT:
        R.compare_exact(got, ref, what)
        print(f"{what}: exact")
    else:
        R.compare_bar(got, ref, mult, plain() if plain is not None and mult not in (None, "f32") else None, what)


def ids(cases, form):
    return [R.case_id(c) + "-" + form(c) for c in cases]


_RB = {}


def rulebook(key, build):
    if key not in _RB:
        _RB[key] = build()
    return _RB[key]


def epi_struct(partial):
    return _lib.BnEpilogue(partial.ptr, None, None, 0.0)


# ---------------------------------------------------------------- msp_conv_tile / msp_conv_tile_bn
TILE = R.tile_cases()


def _tile_form(c):
    return R.tile_form_id(c["V"], c["c_in"], c["c_out"])


@pytest.mark.parametrize("c", TILE, ids=ids(TILE, _tile_form))
def test_conv_tile(c):
    ci, co, K, flip = c["c_in"], c["c_out"], c["K"], c["flip"]
    m, n_in = R.case_map(c)
    V = m.shape[1]
    what = "msp_conv_tile " + R.case_id(c) + " " + _tile_form(c)
    # the restated dispatch against the library's
    assert q("msp_conv_tile_form", V, ci, co, 128) == (1 if R.use_x6r(V, ci, co) else 2), what
    wsb = q("msp_conv_tile_workspace_size", V, K, ci, co, 128)
    assert wsb == R.tile_ws_bytes(V, K, ci, co), (what, wsb)
    tl = rulebook(("tile", id(m)), lambda: R.tile_rulebook(m))
    x, w = R.fwd_data(c["family"], m, n_in, ci, co, flip & 3)
    ref = R.fwd(x, w, m, flip & 3)
    bx, bw = Buf(x), Buf(w)
    bt, bo, bs, br = Buf(tl["tile_start"]), Buf(tl["chunk_off"]), Buf(tl["chunk_src"]), Buf(tl["chunk_row"])
    img = None
    if c.get("image"):      # flip bit 2: the image comes from the library's own image entry
        from sparseconvnet.weight_images import WeightImages
        wt_dev = bw.big[G:G + bw.n].view(torch.float32).view(w.shape)
        wi = WeightImages([wt_dev], DEV)
        assert wi.lookup(0, wt_dev, V, K, ci, co, flip & 3) is None and wi.prepare()
        img = wi.lookup(0, wt_dev, V, K, ci, co, flip & 3)
        assert img is not None and img.numel() >= wsb
    P = -(-V // 128)
    assert q("msp_conv_bn_parts", V) == P

    def run():
        out = Buf(out_floats=V * co)
        ws = Buf(ws=wsb)
        args = [bx.ptr, ci, bw.ptr, K, flip, co, 128, bt.ptr, bo.ptr, bs.ptr, br.ptr, V, out.ptr,
                img.data_ptr() if img is not None else ws.ptr, wsb]
        res = {}
        if c.get("epi"):
            part = Buf(out_doubles=2 * co * (P + 1))
            epi = epi_struct(part)
            call("msp_conv_tile_bn", *args, ctypes.byref(epi))
            part.check(what)
            flat = part.array(F64, (-1,))
            res["partial"] = flat[:2 * co * P].reshape(2, co, P)
            assert not np.isnan(res["partial"]).any(), what + ": an epilogue slot left unwritten"
            assert np.isnan(flat[2 * co * P:]).all(), what + ": the forward epilogue wrote past partial[2][C][P]"
        else:
            call("msp_conv_tile", *args)
        out.check(what)
        ws.check(what)
        res["out"] = out.array(F32, (V, co))
        assert not np.isnan(res["out"]).any(), what + ": output rows left unwritten"
        return res
    got = twice(run, [bx, bw, bt, bo, bs, br], what)
    verdict(c, got["out"], ref, what, 3, lambda: R.plain_fp32(x, w, m, flip & 3))
    if c.get("epi") and c["family"] == "integer":
        assert np.array_equal(got["partial"], R.epi_partial(got["out"])), what + ": epilogue sums"


# ---------------------------------------------------------------- msp_conv_local / msp_conv_local_bn
LOCAL = R.local_cases()


def _local_form(c):
    return f"x6s-NT{R.local_nt(c['c_out'])}"


@pytest.mark.parametrize("c", LOCAL, ids=ids(LOCAL, _local_form))
def test_conv_local(c):
    ci, co, K, flip = c["c_in"], c["c_out"], c["K"], c["flip"]
    m, n_in = R.case_map(c)
    V = m.shape[1]
    what = "msp_conv_local " + R.case_id(c) + " " + _local_form(c)
    wsb = q("msp_conv_local_workspace_size", K, ci, co)
    assert wsb == K * co * (-(-ci // 32) * 32) * 6, what
    d = _lib.WeightImage()
    assert _lib.load().msp_conv_weight_image(1, V, K, ci, co, flip, ctypes.byref(d)) == 0 and d.p == R.local_nt(co)
    shuffle = 1 if c.get("shuffle") else None
    loc = rulebook(("local", id(m), shuffle, bool(c.get("wave_off"))),
                   lambda: R.local_rulebook(m, shuffle=shuffle, wave_off=bool(c.get("wave_off"))))
    if c["kind"] == "wide":
        assert loc["max_u"] > 2 * R.X6S_STAGE
    x, w = R.fwd_data(c["family"], m, n_in, ci, co, flip)
    ref = R.fwd(x, w, m, flip)
    bx, bw = Buf(x), Buf(w)
    bl, bu, br, bp = Buf(loc["lidx"]), Buf(loc["u_start"]), Buf(loc["u_rows"]), Buf(loc["perm"])
    bwo = Buf(loc["wave_off"]) if loc["wave_off"] is not None else None
    P = -(-V // 128)

    def run():
        out = Buf(out_floats=V * co)
        ws = Buf(ws=wsb)
        args = [bx.ptr, ci, bw.ptr, K, flip, co, 128, bl.ptr, bu.ptr, br.ptr, bp.ptr,
                bwo.ptr if bwo is not None else None, V, out.ptr, ws.ptr, wsb]
        res = {}
        if c.get("epi"):
            part = Buf(out_doubles=2 * co * (P + 1))
            epi = epi_struct(part)
            call("msp_conv_local_bn", *args, ctypes.byref(epi))
            part.check(what)
            flat = part.array(F64, (-1,))
            res["partial"] = flat[:2 * co * P].reshape(2, co, P)
            assert not np.isnan(res["partial"]).any(), what + ": an epilogue slot left unwritten"
            assert np.isnan(flat[2 * co * P:]).all(), what + ": the forward epilogue wrote past partial[2][C][P]"
        else:
            call("msp_conv_local", *args)
        out.check(what)
        ws.check(what)
        res["out"] = out.array(F32, (V, co))
        assert not np.isnan(res["out"]).any(), what + ": output rows left unwritten"
        return res
    got = twice(run, [bx, bw, bl, bu, br, bp] + ([bwo] if bwo is not None else []), what)
    verdict(c, got["out"], ref, what, None)
    if c.get("epi") and c["family"] == "integer":
        assert np.array_equal(got["partial"], R.epi_partial(got["out"])), what + ": epilogue sums"


# ---------------------------------------------------------------- msp_conv_nbr
NBR = R.nbr_cases()


def _nbr_form(c):
    return f"x6g-NT{R.pick_tile(c['c_out'] // 16)}"


@pytest.mark.parametrize("c", NBR, ids=ids(NBR, _nbr_form))
def test_conv_nbr(c):
    ci, co, K, flip = c["c_in"], c["c_out"], c["K"], c["flip"]
    m, n_in = R.case_map(c)
    V = m.shape[1]
    what = "msp_conv_nbr " + R.case_id(c) + " " + _nbr_form(c)
    wsb = q("msp_conv_nbr_workspace_size", K, ci, co)
    d = _lib.WeightImage()
    assert _lib.load().msp_conv_weight_image(2, V, K, ci, co, flip, ctypes.byref(d)) == 0
    assert d.p == 16 * R.pick_tile(co // 16) and d.bytes == wsb, what
    x, w = R.fwd_data(c["family"], m, n_in, ci, co, flip)
    ref = R.fwd(x, w, m, flip)
    perm, mp = R.dense_order(m) if c.get("perm") else (None, m)
    bx, bw, bm = Buf(x), Buf(w), Buf(mp)
    bp = Buf(perm) if perm is not None else None

    def run():
        out = Buf(out_floats=V * co)
        ws = Buf(ws=wsb)
        call("msp_conv_nbr", bx.ptr, ci, bw.ptr, K, flip, co, bm.ptr, bp.ptr if bp is not None else None, V, out.ptr,
             ws.ptr, wsb)
        out.check(what)
        ws.check(what)
        o = out.array(F32, (V, co))
        assert not np.isnan(o).any(), what + ": output rows left unwritten"
        return {"out": o}
    got = twice(run, [bx, bw, bm] + ([bp] if bp is not None else []), what)
    verdict(c, got["out"], ref, what, 2, lambda: R.plain_fp32(x, w, m, flip))


# ---------------------------------------------------------------- msp_conv_pairs / msp_conv_pairs_x6
PAIRS = R.pairs_cases()


def _pairs_rb(c):
    m, n_in = R.case_map(c)
    return m, n_in, rulebook(("pairs", id(m)), lambda: R.pair_rulebook(m, swap=c["counts"] is None))


def _pairs_form(c):
    rb = _pairs_rb(c)[2]
    f = R.pairs_form_id if c["entry"] == "pairs" else R.pairs_x6_form_id
    return c["entry"] + "-" + f(rb["n_chunks"], c["c_in"], c["c_out"])


@pytest.mark.parametrize("c", PAIRS, ids=ids(PAIRS, _pairs_form))
def test_conv_pairs(c):
    ci, co = c["c_in"], c["c_out"]
    m, n_in, rb = _pairs_rb(c)
    K = m.shape[0]
    swap = c["counts"] is None
    n_x = m.shape[1] if swap else n_in                  # rows of the input the pairs read
    n_named = n_in if swap else m.shape[1]
    n_out = n_named + 3                                 # three rows no pair names
    what = "msp_conv_" + R.case_id(c) + " " + _pairs_form(c)
    assert len(np.unique(rb["pair_out"])) == rb["total"] == n_named
    x, wt = R.pairs_data(c["family"], K, n_x, ci, co)
    ref = R.pairs(x, wt, rb["pair_in"], rb["pair_out"], rb["off_start"], n_out)
    assert np.isnan(ref[n_named:]).all() and not np.isnan(ref[:n_named]).any()
    bx, bw = Buf(x), Buf(wt)
    bi, bo, bs, bc = Buf(rb["pair_in"]), Buf(rb["pair_out"]), Buf(rb["off_start"]), Buf(rb["chunk_start"])
    x6 = c["entry"] == "pairs_x6"
    wsb = q("msp_conv_pairs_x6_workspace_size", K, ci, co) if x6 else 0
    assert wsb == (K * co * (-(-ci // 32) * 32) * 6 if x6 else 0)

    def run():
        out = Buf(out_floats=n_out * co)
        args = [bx.ptr, ci, bw.ptr, K, co, bi.ptr, bo.ptr, bs.ptr, bc.ptr, rb["n_chunks"], out.ptr]
        if x6:
            ws = Buf(ws=wsb)
            call("msp_conv_pairs_x6", *args, ws.ptr, wsb)
            ws.check(what)
        else:
            call("msp_conv_pairs", *args)
        out.check(what)
        o = out.array(F32, (n_out, co))
        assert np.isnan(o[n_named:]).all(), what + ": a row no pair names was written"
        assert not np.isnan(o[:n_named]).any(), what + ": a named row left unwritten"
        return {"out": o}
    got = twice(run, [bx, bw, bi, bo, bs, bc], what)
    if c["family"] in R.EXACT:
        R.compare_exact(got["out"], ref, what)
    else:      # 1e-5 of the output scale for both pair forms, as tests/test_gpu_ops.py states it
        R.compare_bar(got["out"][:n_named], ref[:n_named], "f32", None, what)


# ---------------------------------------------------------------- msp_conv_wgrad (pair lists)
WGRAD = R.wgrad_cases()


def _wgrad_form(c):
    wa, wb = R.wgrad_x6_tile(c["c_in"], c["c_out"])
    return f"wgrad-x6-WA{wa}-WB{wb}"


@pytest.mark.parametrize("c", WGRAD, ids=ids(WGRAD, _wgrad_form))
def test_conv_wgrad(c):
    ci, co = c["c_in"], c["c_out"]
    m, n_in = R.case_map(c)
    K, V = m.shape
    what = "msp_conv_wgrad " + R.case_id(c) + " " + _wgrad_form(c)
    rb = rulebook(("pairs", id(m)), lambda: R.pair_rulebook(m))
    own = q("msp_wgrad_pieces", rb["total"], K, ci, co)
    assert own == R.wgrad_pieces(rb["total"], K, ci, co), what
    n_pieces = c["n_pieces"] or own
    x, dy = R.wgrad_data(c["family"], m, n_in, ci, co)
    ref = R.wgrad(x, dy, m)
    bx, bd = Buf(x), Buf(dy)
    bi, bo, bs = Buf(rb["pair_in"]), Buf(rb["pair_out"]), Buf(rb["off_start"])

    def run():
        slab = Buf(out_floats=n_pieces * K * ci * co)
        dw = Buf(out_floats=K * ci * co)
        call("msp_conv_wgrad", bx.ptr, ci, bd.ptr, co, bi.ptr, bo.ptr, bs.ptr, K, n_pieces, slab.ptr, dw.ptr)
        slab.check(what)
        dw.check(what)
        o = dw.array(F32, (K, ci, co))
        assert not np.isnan(o).any(), what + ": dW elements left unwritten"
        return {"dw": o}
    got = twice(run, [bx, bd, bi, bo, bs], what)
    verdict(c, got["dw"], ref, what, "f32")


# ---------------------------------------------------------------- msp_conv_wgrad_chunk / msp_conv_wgrad_far
WCHUNK = R.wgrad_chunk_cases()


def _chunk_index(c, m, V, K, what):
    """The chunk weight gradient's index from the library's index entries over the CPU-built rulebooks ->
    (tile_start, chunk_off, chunk_lr, u_start, u_rows, tile rulebook or None, n_far); all inputs checked."""
    n_tiles = -(-V // 128)
    if c["index"] == "tile":
        tl = rulebook(("tile", id(m)), lambda: R.tile_rulebook(m))
        loc = rulebook(("local", id(m), None, True), lambda: R.local_rulebook(m))
        bt, bo, bs, br = Buf(tl["tile_start"]), Buf(tl["chunk_off"]), Buf(tl["chunk_src"]), Buf(tl["chunk_row"])
        bu, bur = Buf(loc["u_start"]), Buf(loc["u_rows"])
        lr = Buf(ws=tl["n_chunks"] * 16 * 4)
        nf = Buf(ws=8)
        call("msp_wgrad_chunk_index", bt.ptr, bs.ptr, br.ptr, V, bu.ptr, bur.ptr, lr.ptr, nf.ptr)
        for b in (bt, bo, bs, br, bu, bur, lr, nf):
            b.check(what + " index")
        n_far = int(nf.array(np.int64, (1,))[0])
        assert n_far == R.far_rules(m, q("msp_wgrad_chunk_cap")), (what, n_far)
        w = lr.array(np.uint32, (-1,))
        pad = tl["chunk_row"] == 128
        assert np.array_equal(w >> 16, tl["chunk_row"]) and int(((w & 0xFFFF) == 0xFFFF)[~pad].sum()) == n_far, what
        return bt, bo, lr, bu, bur, (bs, br), n_far
    shuffle = 1 if c["index"] == "local-shuffled" else None
    loc = rulebook(("local", id(m), shuffle, True), lambda: R.local_rulebook(m, shuffle=shuffle))
    assert loc["max_u"] <= q("msp_wgrad_chunk_cap")
    bl, bp, bu, bur = Buf(loc["lidx"]), Buf(loc["perm"]), Buf(loc["u_start"]), Buf(loc["u_rows"])
    wsb = q("msp_tile_local_workspace_size", V, 128)
    ws = Buf(ws=wsb)
    bt = Buf(ws=(n_tiles + 2) * 8)
    call("msp_local_chunk_index", bl.ptr, bp.ptr, K, V, bt.ptr, None, None, 0, ws.ptr, wsb)
    ts = bt.array(np.int64, (-1,))
    exp = R.tile_rulebook(m)["tile_start"]          # the same chunk counts: ceil(present / 16) per (tile, offset)
    assert np.array_equal(ts, exp), what + ": msp_local_chunk_index counts"
    total = int(ts[n_tiles])
    bo, lr = Buf(ws=total), Buf(ws=total * 16 * 4)
    call("msp_local_chunk_index", bl.ptr, bp.ptr, K, V, bt.ptr, bo.ptr, lr.ptr, total, ws.ptr, wsb)
    for b in (bl, bp, bu, bur, ws, bt, bo, lr):
        b.check(what + " index")
    return bt, bo, lr, bu, bur, None, 0


def _chunk_form(c):
    """x6c with the 27-offset deal table or round-robin offsets, plus msp_conv_wgrad_far where the map has far rules."""
    far = R.far_rules(R.case_map(c)[0]) > 0 and c["index"] == "tile"
    return "x6c" + ("-deal27" if c["K"] == 27 else "-robin") + ("-far" if far else "")


@pytest.mark.parametrize("c", WCHUNK, ids=ids(WCHUNK, _chunk_form))
def test_conv_wgrad_chunk(c):
    ci, co, K = c["c_in"], c["c_out"], c["K"]
    m, n_in = R.case_map(c)
    V = m.shape[1]
    n_tiles = -(-V // 128)
    what = "msp_conv_wgrad_chunk " + R.case_id(c)
    assert q("msp_wgrad_chunk_ok", V, K, ci, co) == 1 and q("msp_wgrad_chunk_cap") == R.WCHUNK_CAP
    own = q("msp_wgrad_chunk_ranges", V, ci, co)
    assert 1 <= own <= n_tiles, (what, own)
    n_ranges = {1: 1, 0: n_tiles, -1: own}[c["ranges"]]
    bt, bo, lr, bu, bur, far_src, n_far = _chunk_index(c, m, V, K, what)
    assert (n_far > 0) == _chunk_form(c).endswith("-far"), what
    assert n_far > 0 or c["kind"] != "wide", what      # the wide map's tiles pass the staging cap
    x, dy = R.wgrad_data(c["family"], m, n_in, ci, co)
    ref = R.wgrad(x, dy, m)
    bx, bd = Buf(x), Buf(dy)
    far = None
    if n_far:
        fwb = q("msp_wgrad_far_workspace_size", n_far)
        fk, ft, fws = Buf(ws=n_far * 8), Buf(ws=n_far * 4), Buf(ws=fwb)
        call("msp_wgrad_far_list", bt.ptr, bo.ptr, lr.ptr, V, n_far, fk.ptr, ft.ptr, fws.ptr, fwb)
        for b in (fk, ft, fws):
            b.check(what + " far list")
        key = fk.array(np.int64, (-1,))
        w = lr.array(np.uint32, (-1,))
        e = np.nonzero(((w & 0xFFFF) == 0xFFFF) & ((w >> 16) < 128))[0]
        off = bo.array(np.uint8, (-1,)).astype(np.int64)[e // 16]
        assert np.array_equal(key, np.sort((off << 40) | e)), what + ": far list"
        far = (fk, ft)

    def run():
        slab = Buf(out_floats=n_ranges * K * ci * co)
        dw = Buf(out_floats=K * ci * co)
        call("msp_conv_wgrad_chunk", bx.ptr, ci, bd.ptr, co, K, 128, bt.ptr, bo.ptr, lr.ptr, bu.ptr, bur.ptr, V,
             n_ranges, slab.ptr, dw.ptr)
        if far:
            call("msp_conv_wgrad_far", bx.ptr, ci, bd.ptr, co, K, far_src[0].ptr, far_src[1].ptr, far[0].ptr,
                 far[1].ptr, n_far, dw.ptr)
        slab.check(what)
        dw.check(what)
        o = dw.array(F32, (K, ci, co))
        assert not np.isnan(o).any(), what + ": dW elements left unwritten"
        return {"dw": o}
    got = twice(run, [bx, bd, bt, bo, lr, bu, bur] + (list(far_src) + list(far) if far else []), what)
    verdict(c, got["dw"], ref, what, None)


# ---------------------------------------------------------------- msp_conv_narrow_in / msp_conv_wgrad_narrow_in
NARROW = R.narrow_cases()


@pytest.mark.parametrize("c", NARROW, ids=ids(NARROW, lambda c: f"narrow-{c['c_in']}x{c['c_out']}"))
def test_conv_narrow_in(c):
    ci, co, K = c["c_in"], c["c_out"], c["K"]
    m, n_in = R.case_map(c)
    V = m.shape[1]
    what = "msp_conv_narrow_in " + R.case_id(c)
    assert q("msp_conv_narrow_in_ok", K, ci, co) == 1
    own = q("msp_conv_wgrad_narrow_parts", V, K, ci, co)
    assert own == R.narrow_parts(V), what
    bm = Buf(m)
    if not c.get("wgrad_only"):
        x, w = R.fwd_data(c["family"], m, n_in, ci, co, 2)      # wt [K][c_in][c_out], the module's layout
        ref = R.fwd(x, w, m, 2)
        bx, bw = Buf(x), Buf(w)

        def run():
            out = Buf(out_floats=V * co)
            call("msp_conv_narrow_in", bx.ptr, ci, bw.ptr, K, co, bm.ptr, V, out.ptr)
            out.check(what)
            o = out.array(F32, (V, co))
            assert not np.isnan(o).any(), what + ": output rows left unwritten"
            return {"out": o}
        got = twice(run, [bx, bw, bm], what)
        R.compare_exact(got["out"], ref, what)
    if c["n_parts"] is None:
        return
    n_parts = {0: own, -1: V + 3}.get(c["n_parts"], c["n_parts"])
    x, dy = R.wgrad_data(c["family"], m, n_in, ci, co)
    ref = R.wgrad(x, dy, m)
    bx, bd = Buf(x), Buf(dy)
    what = "msp_conv_wgrad_narrow_in " + R.case_id(c) + f" parts {n_parts}"

    def run_w():
        slab = Buf(out_floats=n_parts * K * ci * co)
        dw = Buf(out_floats=K * ci * co)
        call("msp_conv_wgrad_narrow_in", bx.ptr, ci, bd.ptr, co, bm.ptr, K, V, n_parts, slab.ptr, dw.ptr)
        slab.check(what)
        dw.check(what)
        o = dw.array(F32, (K, ci, co))
        assert not np.isnan(o).any(), what + ": dW elements left unwritten"
        return {"dw": o}
    got = twice(run_w, [bx, bd, bm], what)
    R.compare_exact(got["dw"], ref, what)


# ---------------------------------------------------------------- error paths (return code and message only)
def test_error_paths():
    """Every call below must be rejected by the entry's argument checks before anything is launched, so some
    pointer arguments are mere non-NULL placeholders of the wrong type; never copy that into a call that runs."""
    V, K, ci, co = 129, 27, 48, 48
    m, n_in = R.make_map("ragged", K, V)
    tl, loc = R.tile_rulebook(m), R.local_rulebook(m)
    x, w = R.fwd_data("integer", m, n_in, ci, co, 0)
    bx, bw, bm = Buf(x), Buf(w), Buf(m)
    bt, bo, bs, br = Buf(tl["tile_start"]), Buf(tl["chunk_off"]), Buf(tl["chunk_src"]), Buf(tl["chunk_row"])
    bl, bu, bur, bp, bwo = (Buf(loc[k]) for k in ("lidx", "u_start", "u_rows", "perm", "wave_off"))
    out = Buf(out_floats=V * 64)
    ws = Buf(ws=1 << 22)
    big = 1 << 22

    def tile(ci=ci, co=co, K=K, flip=0, wsb=big):
        return ("msp_conv_tile", bx.ptr, ci, bw.ptr, K, flip, co, 128, bt.ptr, bo.ptr, bs.ptr, br.ptr, V, out.ptr,
                ws.ptr, wsb)

    def local(ci=ci, co=co, K=K, flip=0, wsb=big):
        return ("msp_conv_local", bx.ptr, ci, bw.ptr, K, flip, co, 128, bl.ptr, bu.ptr, bur.ptr, bp.ptr, bwo.ptr, V,
                out.ptr, ws.ptr, wsb)

    def nbr(ci=ci, co=co, K=K, flip=0, wsb=big):
        return ("msp_conv_nbr", bx.ptr, ci, bw.ptr, K, flip, co, bm.ptr, None, V, out.ptr, ws.ptr, wsb)
    # a workspace one byte short, for each entry that takes one (the shared-tile and the per-wave form both)
    for f, size in ((tile, q("msp_conv_tile_workspace_size", V, K, ci, co, 128)),
                    (local, q("msp_conv_local_workspace_size", K, ci, co)),
                    (nbr, q("msp_conv_nbr_workspace_size", K, ci, co))):
        name, *args = f(wsb=size - 1)
        fails(name, "workspace too small", *args)
    name, *args = tile(ci=32, co=32, wsb=q("msp_conv_tile_workspace_size", V, K, 32, 32, 128) - 1)
    fails(name, "workspace too small", *args)
    rb = R.pair_rulebook(R.make_single_map((5, 17), 30)[0])
    bi, bq, bss, bc = Buf(rb["pair_in"]), Buf(rb["pair_out"]), Buf(rb["off_start"]), Buf(rb["chunk_start"])
    fails("msp_conv_pairs_x6", "workspace too small", bx.ptr, 16, bw.ptr, 2, 16, bi.ptr, bq.ptr, bss.ptr, bc.ptr,
          rb["n_chunks"], out.ptr, ws.ptr, q("msp_conv_pairs_x6_workspace_size", 2, 16, 16) - 1)
    fails("msp_wgrad_far_list", "workspace too small", bt.ptr, bo.ptr, bs.ptr, V, 5, ws.ptr, ws.ptr, ws.ptr,
          q("msp_wgrad_far_workspace_size", 5) - 1)
    fails("msp_local_chunk_index", "workspace too small", bl.ptr, bp.ptr, K, V, ws.ptr, None, None, 0, ws.ptr,
          q("msp_tile_local_workspace_size", V, 128) - 1)
    fails("msp_conv_wgrad_chunk", "multiples of 32", bx.ptr, 48, bx.ptr, 32, K, 128, bt.ptr, bo.ptr, bs.ptr, bu.ptr,
          bur.ptr, V, 1, ws.ptr, out.ptr)
    fails("msp_conv_wgrad_far", "multiples of 32", bx.ptr, 32, bx.ptr, 48, K, bs.ptr, br.ptr, ws.ptr, ws.ptr, 1,
          out.ptr)
    # channels not a multiple of 16
    for f in (tile, local, nbr):
        for kw in (dict(ci=40), dict(co=24)):
            name, *args = f(**kw)
            fails(name, "multiples of 16", *args)
    fails("msp_conv_pairs", "multiples of 16", bx.ptr, 24, bw.ptr, 2, 16, bi.ptr, bq.ptr, bss.ptr, bc.ptr,
          rb["n_chunks"], out.ptr)
    fails("msp_conv_wgrad", "multiples of 16", bx.ptr, 16, bx.ptr, 24, bi.ptr, bq.ptr, bss.ptr, 2, 1, ws.ptr, out.ptr)
    # K beyond what an entry takes, flip beyond its three bits
    for f, k in ((tile, 129), (nbr, 129), (local, 28)):
        name, *args = f(K=k)
        fails(name, "K must be in", *args)
        name, *args = f(flip=8)
        fails(name, "flip must be 0..7", *args)
    # the narrow-input entries take c_out 16, 32 and 64 only
    fails("msp_conv_narrow_in", "needs K <= 27", bx.ptr, 3, bw.ptr, 27, 48, bm.ptr, V, out.ptr)
    fails("msp_conv_wgrad_narrow_in", "needs K <= 27", bx.ptr, 3, bx.ptr, 48, bm.ptr, 27, V, 1, ws.ptr, out.ptr)
    for b in (bx, bw, bm, bt, bo, bs, br, bl, bu, bur, bp, bwo, out, ws):
        b.check("error paths")
    assert np.isnan(out.array(F32, (-1,))).all(), "a rejected call wrote its output"
