"""The pseudo-label training tail on the voxel rows: msp_voxel_ce_fwd / _bwd, ops.VoxelCrossEntropyFunction and
SparseConvBase_.point_loss / FullySupervised.point_loss.

The reference is the formula of utils/loss.py:29-33 and models/MultiLabelContrastive.py:88-94 in fp64 with torch
on the CPU,

    z = (x64 @ W64.T + b64)[p2v]
    F.cross_entropy(z[keep], labels[keep]) + sum(gscene * per-scene means of z)

with autograd for the gradients.  The mean of a scene without points is taken as 0, as msp_scene_mean_fwd
defines it (torch's mean over nothing is NaN); only the V = 1, B = 3 case has such scenes.

Bars (tests/test_gpu_pseudo.py::test_point_ce_against_fp64_fixture): loss within 1e-5 max(1, |ref|), gradients
within 1e-5 max|ref grad|, scene logits within 1e-5 max(1, max|ref|)."""
import types

import pytest
import torch
import torch.nn.functional as F

from sparseconvnet import _lib, graphs, ops
from sparseconvnet._lib import ptr
from wsss3d import (EasyDict, LOSS_REGISTRY, MODEL_REGISTRY, get_pseudo_labels, point_cross_entropy, segment_mean,
                    voxel_point_cross_entropy)
from wsss3d.synthetic import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG2 = 5  # level-0 spatial size 32: batch = key >> 15
C_IN = 16
HEAVY = 300  # points of the crowded voxel: more than a wave (64) and more than a block (256) of point lanes


class Case:
    """V voxels in B scenes built directly: one or two points per voxel and one voxel of HEAVY points, the points
    of a scene contiguous in point order and shuffled inside it, ~30 % of the labels -100."""

    def __init__(self, V, C, B, seed, ignore=0.3):
        g = torch.Generator().manual_seed(seed)
        self.V, self.C, self.B = V, C, B
        cnt = torch.randint(1, 3, (V,), generator=g)
        cnt[V // 2] = HEAVY
        # scene boundaries away from the multiples of 64 (V >= 63: rows 22 / 45 or 88 / 173 ...)
        cuts = [0] + [min(V, (V * k) // B + k) for k in range(1, B)] + [V]
        self.v2b = torch.repeat_interleave(torch.arange(B), torch.tensor(cuts[1:]) - torch.tensor(cuts[:-1]))
        vstart = torch.zeros(V + 1, dtype=torch.int64)
        vstart[1:] = cnt.cumsum(0)
        self.N = N = int(vstart[-1])
        self.offsets = [int(vstart[c]) for c in cuts]
        perm = torch.empty(N, dtype=torch.int64)
        for b in range(B):  # sorted position j -> point id, a shuffle inside the scene's point range
            lo, hi = self.offsets[b], self.offsets[b + 1]
            perm[lo:hi] = lo + torch.randperm(hi - lo, generator=g)
        self.p2v = torch.empty(N, dtype=torch.int64)
        self.p2v[perm] = torch.repeat_interleave(torch.arange(V), cnt)
        self.labels = torch.randint(0, C, (N,), generator=g)
        self.labels[torch.rand(N, generator=g) < ignore] = -100
        self.x = torch.randn(V, C_IN, generator=g)
        self.W = torch.randn(C, C_IN, generator=g) * 0.5
        self.b = torch.randn(C, generator=g)
        self.gscene = torch.randn(B, C, generator=g)
        self.rules = types.SimpleNamespace(n_points=N, perm=perm.to(torch.int32).to(DEV),
                                           p2v=self.p2v.to(torch.int32).to(DEV),
                                           vstart=vstart.to(torch.int32).to(DEV))
        keys = (self.v2b << (3 * LOG2)) | torch.arange(V)
        self.level = types.SimpleNamespace(keys=keys.to(DEV), log2=LOG2)  # int64 bits = the uint64 keys

    def scene_means(self, z):
        """(B, C) per-scene means of the point rows z; 0 for a scene without points."""
        return torch.stack([z[self.offsets[b]:self.offsets[b + 1]].sum(0) /
                            max(self.offsets[b + 1] - self.offsets[b], 1) for b in range(self.B)])

    def reference(self, labels=None, bias=True, gscene=True):
        """fp64: (loss, scene logits, grads of loss + sum(gscene * scene) w.r.t. x, W, b, and w.r.t. the voxel
        rows).  No kept label: loss NaN and only the scene term in the gradients."""
        labels = self.labels if labels is None else labels
        x, W, b = (t.double().requires_grad_(True) for t in (self.x, self.W, self.b))
        vl = x @ W.T
        vl.retain_grad()
        z = (vl + b if bias else vl)[self.p2v]
        keep = (labels >= 0) & (labels < self.C)
        scene = self.scene_means(z)
        total = (self.gscene.double() * scene).sum() if gscene else z.sum() * 0
        loss = F.cross_entropy(z[keep], labels[keep]) if keep.any() else torch.tensor(float("nan")).double()
        if keep.any():
            total = total + loss
        total.backward()
        return loss.item(), scene.detach(), (x.grad, W.grad, b.grad if bias else None), vl.grad


def _close(got, ref, what):
    err = (got.detach().double().cpu() - ref).abs().max().item() if ref.numel() else 0.0
    scale = ref.abs().max().item() if ref.numel() else 0.0
    print(f"  {what}: max err {err:.3e} of {scale:.3e}")
    assert err <= 1e-5 * scale, what


def _close_values(got, ref, what):
    err = (got.detach().double().cpu() - ref).abs().max().item()
    print(f"  {what}: max err {err:.3e} of {ref.abs().max().item():.3e}")
    assert err <= 1e-5 * max(1.0, ref.abs().max().item()), what


def _close_loss(loss, ref):
    print(f"  loss {loss.item():.8f} ref {ref:.8f}")
    assert abs(loss.item() - ref) <= 1e-5 * max(1.0, abs(ref))


def _kernels(case, vl, bias, labels, gscene, gout=1.0):
    """msp_voxel_ce_fwd + _bwd on the padded rows vl (V, ld) -> (loss, n_kept, n_bad, dvl)."""
    V, ld = vl.shape
    s = _lib.stream(vl.device)
    r = case.rules
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    nums = torch.empty(2, dtype=torch.int64, device=DEV)
    lse = torch.empty(V, dtype=torch.float32, device=DEV)
    kept = torch.empty(V, dtype=torch.int32, device=DEV)
    wsb = int(_lib.query("msp_voxel_ce_workspace_size", V))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _lib.call("msp_voxel_ce_fwd", ptr(vl), V, ld, case.C, ptr(bias), ptr(r.perm), ptr(r.vstart), ptr(labels), case.N,
              ptr(loss), ptr(nums), ptr(nums[1:]), ptr(lse), ptr(kept), ptr(ws), wsb, s)
    npts = torch.tensor([case.offsets[b + 1] - case.offsets[b] for b in range(case.B)], device=DEV)
    g = torch.tensor(gout, dtype=torch.float32, device=DEV)
    dvl = torch.full_like(vl, float("nan"))
    _lib.call("msp_voxel_ce_bwd", ptr(vl), V, ld, case.C, ptr(bias), ptr(r.perm), ptr(r.vstart), ptr(labels), case.N,
              ptr(lse), ptr(kept), ptr(nums), ptr(g), ptr(gscene), ptr(case.level.keys), 3 * LOG2, case.B, ptr(npts),
              ptr(dvl), s)
    return loss, int(nums[0]), int(nums[1]), dvl, kept


def _fused(case, labels, bias=True, gscene=True):
    x, W, b = (t.to(DEV).requires_grad_(True) for t in (case.x, case.W, case.b))
    scene, loss, n_kept, n_bad = voxel_point_cross_entropy(x, W, b if bias else None, labels.to(DEV), case.level,
                                                           case.rules, case.B, return_counts=True)
    total = loss + ((case.gscene.to(DEV) * scene).sum() if gscene else 0)
    total.backward()
    return loss.detach(), scene.detach(), (x.grad, W.grad, b.grad if bias else None), int(n_kept), int(n_bad)


def _point_path(case, labels, bias=True):
    """PointLogitsFunction + segment_mean + point_cross_entropy; scenes without points are left out of the sum
    (their mean is NaN here)."""
    x, W, b = (t.to(DEV).requires_grad_(True) for t in (case.x, case.W, case.b))
    logits = ops.PointLogitsFunction.apply(x, W, b if bias else None, case.rules)
    scene = segment_mean(logits, case.offsets)
    loss, n_kept, n_bad = point_cross_entropy(logits, labels.to(DEV), return_counts=True)
    ne = torch.tensor([case.offsets[k + 1] > case.offsets[k] for k in range(case.B)], device=DEV)
    (loss + (case.gscene.to(DEV)[ne] * scene[ne]).sum()).backward()
    scene = torch.where(ne[:, None], scene.detach(), torch.zeros_like(scene))
    return loss.detach(), scene, (x.grad, W.grad, b.grad if bias else None), int(n_kept), int(n_bad)


def _check(out, ref, case, labels, bias):
    loss, scene, grads, n_kept, n_bad = out
    ref_loss, ref_scene, ref_grads, _ = ref
    keep = (labels >= 0) & (labels < case.C)
    assert n_kept == int(keep.sum()) and n_bad == int(((labels != -100) & ~keep).sum())
    _close_loss(loss, ref_loss)
    _close_values(scene, ref_scene, "scene logits")
    for got, want, name in zip(grads, ref_grads, ("dx", "dW", "db")):
        if want is not None:
            _close(got, want, name)


@pytest.mark.parametrize("C", [1, 7, 20, 64])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_kernels_and_function_against_fp64(V, C):
    """Tile and wave edges in the voxel rows (one row; one wave less one, one wave, one more; one 256-row tile and
    one more, two 128-row tiles and one more at C = 64), every class count the staging treats differently with
    row strides 16 / 32 / 64, a voxel of 300 points, one and three scenes, with and without gscene / bias.  The
    kernels on their own on rows whose padding columns hold garbage, then the autograd Function."""
    for B in (1, 3):
        case = Case(V, C, B, seed=1000 * V + 10 * C + B)
        labels = case.labels.to(DEV)
        for full in (True, False):
            print(f"V={V} C={C} B={B} N={case.N} {'bias + gscene' if full else 'plain'}")
            ref = case.reference(bias=full, gscene=full)
            ld = ops._pad16(C)
            vl = torch.full((V, ld), 1e3)
            vl[:, :C] = case.x @ case.W.T
            vl = vl.to(DEV)
            ref_vl = vl[:, :C].double().cpu().requires_grad_(True)
            z = (ref_vl + case.b.double() if full else ref_vl)[case.p2v]
            keep = case.labels != -100
            ref_k = F.cross_entropy(z[keep], case.labels[keep])
            (ref_k + ((case.gscene.double() * case.scene_means(z)).sum() if full else 0)).backward()
            bias = case.b.to(DEV) if full else None
            gs = case.gscene.to(DEV) if full else None
            loss, n_kept, n_bad, dvl, kept = _kernels(case, vl, bias, labels, gs)
            assert n_kept == int(keep.sum()) and n_bad == 0
            assert torch.equal(kept.cpu().long(), torch.zeros(V, dtype=torch.int64).index_add_(
                0, case.p2v, keep.long()))
            _close_loss(loss, ref_k.item())
            _close(dvl[:, :C], ref_vl.grad, "dvl")
            assert (dvl[:, C:] == 0).all(), "padding columns of dvl"
            loss2, _, _, dvl2, _ = _kernels(case, vl, bias, labels, gs)
            assert torch.equal(loss, loss2) and torch.equal(dvl, dvl2)
            out = _fused(case, case.labels, bias=full, gscene=full)
            _check(out, ref, case, case.labels, full)
            out2 = _fused(case, case.labels, bias=full, gscene=full)
            assert torch.equal(out[0], out2[0]) and torch.equal(out[1], out2[1])
            assert all(a is None or torch.equal(a, b) for a, b in zip(out[2], out2[2]))


def test_too_many_classes_is_a_clean_error():
    case = Case(5, 7, 1, seed=3)
    with pytest.raises(ValueError, match="at most 64"):
        voxel_point_cross_entropy(case.x.to(DEV), torch.zeros(65, C_IN, device=DEV), None, case.labels.to(DEV),
                                  case.level, case.rules, 1)
    with pytest.raises(RuntimeError, match="msp_voxel_ce_fwd: C=65"):
        _lib.call("msp_voxel_ce_fwd", None, 5, 80, 65, None, None, None, None, 5, None, None, None, None, None, None,
                  0, None)


def test_ignored_and_bad_labels():
    case = Case(65, 20, 3, seed=11)
    # every label -100: NaN loss, no CE gradient, the scene term as in the reference
    none = torch.full((case.N,), -100, dtype=torch.int64)
    ref = case.reference(labels=none)
    loss, scene, grads, n_kept, n_bad = _fused(case, none)
    assert torch.isnan(loss) and n_kept == 0 and n_bad == 0
    _close_values(scene, ref[1], "scene logits")
    for got, want, name in zip(grads, ref[2], ("dx", "dW", "db")):
        _close(got, want, name)
    _, _, plain, _, _ = _fused(case, none, gscene=False)
    assert all((g == 0).all() for g in plain), "CE part of the gradient with nothing kept"
    vl = (case.x @ case.W.T).to(DEV)
    vl = F.pad(vl, (0, 32 - 20))
    _, _, _, dvl, kept = _kernels(case, vl, case.b.to(DEV), none.to(DEV), None)
    assert (dvl == 0).all() and (kept == 0).all()
    # labels 20 and -5 among valid ones: counted as bad, never used as an index
    bad = case.labels.clone()
    valid = (bad >= 0).nonzero().flatten()
    bad[valid[0]], bad[valid[-1]] = 20, -5
    out = _fused(case, bad)
    assert out[4] == 2 and torch.isfinite(out[0]) and all(torch.isfinite(g).all() for g in out[2])
    _check(out, case.reference(labels=bad), case, bad, True)
    # a voxel whose points are all ignored next to one whose points carry two different classes (the crowded
    # voxel's neighbour gets a second class by hand)
    lab = case.labels.clone()
    v_ign, v_two = case.V // 2 + 1, case.V // 2
    lab[case.p2v == v_ign] = -100
    pts = (case.p2v == v_two).nonzero().flatten()
    lab[pts] = 3
    lab[pts[::2]] = 17
    out = _fused(case, lab)
    _check(out, case.reference(labels=lab), case, lab, True)
    _, _, _, dvl, kept = _kernels(case, vl, case.b.to(DEV), lab.to(DEV), None)
    assert int(kept[v_ign]) == 0 and (dvl[v_ign] == 0).all() and int(kept[v_two]) == HEAVY
    assert dvl[v_two, 3] < 0 or dvl[v_two, 17] < 0


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_agrees_with_the_point_path(V):
    for B in (1, 3):
        case = Case(V, 20, B, seed=1000 * V + 200 + B)
        lab = case.labels.clone()
        lab[0] = 20  # a bad label: both paths count it
        ref = case.reference(labels=lab)
        fused, point = _fused(case, lab), _point_path(case, lab)
        print(f"V={V} B={B}: fused")
        _check(fused, ref, case, lab, True)
        print(f"V={V} B={B}: per point")
        _check(point, ref, case, lab, True)
        assert fused[3:] == point[3:]


def _model_and_batch():
    torch.manual_seed(1)
    b = make_batch(2, 20, seed=6, spacing=0.04)
    pc = EasyDict(name="SparseConvUNet", m=16, dimension=3, full_scale=4096, block_reps=1, residual_blocks=True)
    model = MODEL_REGISTRY.get("FullySupervised")[0](pc).to(DEV)
    with torch.no_grad():
        model.linear.bias.uniform_(-0.5, 0.5)
    x = EasyDict(coords=torch.from_numpy(b["coords"]).to(DEV), feature=torch.from_numpy(b["feats"]).to(DEV),
                 batch_offsets=b["batch_offsets"])
    return model, x, b


def _count_calls(monkeypatch):
    seen = {}
    real = ops.call

    def counting(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(ops, "call", counting)
    return seen


def test_training_step_end_to_end(monkeypatch):
    """test_pseudo_label_training_step_end_to_end's setting; the step's loss is the scene-level soft margin loss
    plus the point loss, once through model.point_loss and once through forward(istrain=True) + Classification.
    Every parameter gradient within 1e-4 scale + 1e-9 (that test's bar)."""
    model, x, b = _model_and_batch()
    model.eval()
    with torch.no_grad():
        logits = model(x)
    y = torch.from_numpy(b["scene_labels"]).to(DEV)
    labels, num = get_pseudo_labels(logits, y, b["batch_offsets"], 0.6)
    assert int(num) > 0
    model.train()
    seen = _count_calls(monkeypatch)
    model.zero_grad(set_to_none=True)
    scene, point, n_kept, n_bad = model.point_loss(x, labels, return_counts=True)
    lf = F.multilabel_soft_margin_loss(scene, y) + point
    lf.backward()
    assert seen.get("msp_voxel_ce_fwd") == 1 and seen.get("msp_voxel_ce_bwd") == 1
    assert "msp_point_rows_bias" not in seen and "msp_output_bwd" not in seen, sorted(seen)
    assert int(n_kept) == int(num) and int(n_bad) == 0
    gf = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    seen.clear()
    model.zero_grad(set_to_none=True)
    scene_ref, point_logits = model((x, None), istrain=True)
    cls = LOSS_REGISTRY.get("Classification")[0]
    lr = cls(scene_ref, y) + cls(point_logits, labels)
    lr.backward()
    assert "msp_point_rows_bias" in seen and "msp_output_bwd" in seen  # the counter sees the per-point path
    print(f"loss {lf.item():.8f} ref {lr.item():.8f}")
    assert abs(lf.item() - lr.item()) <= 1e-5 * max(1.0, abs(lr.item()))
    for k, p in model.named_parameters():
        scale = max(p.grad.abs().max().item(), 1e-12)
        assert (gf[k] - p.grad).abs().max().item() <= 1e-4 * scale + 1e-9, k


def test_fallback_is_the_per_point_path(monkeypatch):
    """Two scenes' points interleaved: batch_offsets do not describe the batch column, so point_loss takes the
    per-point path and returns exactly what that path returns when called directly."""
    model, x, b = _model_and_batch()
    g = torch.Generator().manual_seed(4)
    shuffle = torch.randperm(x.coords.size(0), generator=g).to(DEV)
    x = EasyDict(coords=x.coords[shuffle], feature=x.feature[shuffle], batch_offsets=b["batch_offsets"])
    labels = torch.randint(0, 20, (len(shuffle),), generator=g)
    labels[torch.rand(len(shuffle), generator=g) < 0.3] = -100
    labels = labels.to(DEV)
    model.eval()
    seen = _count_calls(monkeypatch)
    with torch.no_grad():
        scene, loss, n_kept, n_bad = model.point_loss(x, labels, return_counts=True)
        assert "msp_voxel_ce_fwd" not in seen and "msp_point_rows_bias" in seen
        logits = model.pc_encoder.point_logits(x, model.linear)
        ref_scene = segment_mean(logits, x.batch_offsets)
        ref_loss, ref_kept, ref_bad = point_cross_entropy(logits, labels, return_counts=True)
        scene2, loss2 = model.point_loss(x, labels)
    assert torch.equal(scene, ref_scene) and torch.equal(loss, ref_loss)
    assert torch.equal(scene2, ref_scene) and torch.equal(loss2, ref_loss)
    assert int(n_kept) == int(ref_kept) == int((labels != -100).sum()) and int(n_bad) == int(ref_bad) == 0


def test_step_is_capturable_and_makes_no_host_read():
    """Forward + backward from static voxel rows and labels captured once on one stream (no parallel branches);
    replayed on labels with a different number of -100s, every output is bit-equal to the eager call on those
    labels.  Under torch's sync-debug mode the eager call raises nothing."""
    case = Case(257, 20, 3, seed=21)
    lab_a = case.labels.to(DEV)
    lab_b = lab_a.clone()
    lab_b[::3] = -100
    assert int((lab_a == -100).sum()) != int((lab_b == -100).sum())
    x, W, bias = (t.to(DEV).requires_grad_(True) for t in (case.x, case.W, case.b))
    gs = case.gscene.to(DEV)
    y = lab_a.clone()

    def body(labels=y):
        scene, loss = voxel_point_cross_entropy(x, W, bias, labels, case.level, case.rules, case.B)
        grads = torch.autograd.grad(loss + (gs * scene).sum(), (x, W, bias))
        return (scene, loss) + grads

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        body()  # warm-up outside the capture
    g, outs = graphs.capture(body, stream)
    torch.cuda.current_stream().wait_stream(stream)
    for labels in (lab_b, lab_a):
        y.copy_(labels)
        g.replay()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            eager = body(labels)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for got, want in zip(outs, eager):
            assert torch.equal(got, want)


def test_no_point_sized_allocation():
    """200k points on 60k voxels: forward + backward of the fused tail allocate less than one (N, 20) fp32 tensor
    above what was held before the call; the per-point path on the same inputs allocates more than two (the
    control: the assertion can fail)."""
    g = torch.Generator().manual_seed(8)
    V, N, C = 60000, 200000, 20
    cnt = 1 + torch.bincount(torch.randint(0, V, (N - V,), generator=g), minlength=V)
    vstart = torch.zeros(V + 1, dtype=torch.int64)
    vstart[1:] = cnt.cumsum(0)
    perm = torch.randperm(N, generator=g)
    p2v = torch.empty(N, dtype=torch.int64)
    p2v[perm] = torch.repeat_interleave(torch.arange(V), cnt)
    rules = types.SimpleNamespace(n_points=N, perm=perm.to(torch.int32).to(DEV), p2v=p2v.to(torch.int32).to(DEV),
                                  vstart=vstart.to(torch.int32).to(DEV))
    level = types.SimpleNamespace(keys=torch.arange(V, device=DEV), log2=7)  # one scene: V < 2^21
    labels = torch.randint(0, C, (N,), generator=g)
    labels[torch.rand(N, generator=g) < 0.3] = -100
    labels = labels.to(DEV)
    x = torch.randn(V, C_IN, generator=g).to(DEV).requires_grad_(True)
    W = (torch.randn(C, C_IN, generator=g) * 0.5).to(DEV).requires_grad_(True)
    b = torch.randn(C, generator=g).to(DEV).requires_grad_(True)
    one = N * C * 4

    def fused():
        scene, loss = voxel_point_cross_entropy(x, W, b, labels, level, rules, 1)
        return scene, loss

    def per_point():
        logits = ops.PointLogitsFunction.apply(x, W, b, rules)
        return segment_mean(logits, [0, N]), point_cross_entropy(logits, labels)

    peaks, values = [], []
    for tail in (fused, per_point, fused):  # the first run also warms the caches that persist (arange, queries)
        x.grad = W.grad = b.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        scene, loss = tail()
        (loss + scene.sum()).backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        values.append((loss.item(),))
        del scene, loss
    print(f"(N, 20) fp32 = {one} B; peak above baseline: fused {peaks[2]} B, per point {peaks[1]} B")
    assert peaks[2] < one
    assert peaks[1] > 2 * one
    # the same inputs went through both: each loss is within 1e-5 max(1, |ref|) of fp64 (the tests above)
    assert abs(values[2][0] - values[1][0]) <= 2e-5 * max(1.0, abs(values[1][0]))
