"""The pseudo-label stage on the device: msp_pseudo_labels / msp_confusion / msp_point_ce_* and their wsss3d
wrappers against the fixture made by the reference's own utils/stats.py, utils/iou.py and an fp64
F.cross_entropy (tests/golden/make_pseudo_golden.py), against an fp64 restatement of the formula on odd shapes,
captured into a graph, and end to end behind FullySupervised.

Near rows.  fp32 cannot decide a comparison whose fp64 margin is below its own rounding: a row is *near* when,
in fp64, its two largest confidences differ by < 1e-6 while the masked fp32 inputs do not tie exactly, or when
its largest confidence is within 1e-6 of the threshold without being the exact 0.5 of a masked class.  Labels
must be equal on every other row, exact ties (first index) and exact-0.5 rows (labelled at threshold 0.5)
included, and near rows may be at most 0.5 % of the rows; the reference's own fp32 run has none on the
fixture, and none of the random cases below has one."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sparseconvnet import graphs, ops
from wsss3d import (EasyDict, LOSS_REGISTRY, MODEL_REGISTRY, PseudoLabelPass, assess_label_quality,
                    get_pseudo_labels, point_cross_entropy)
from wsss3d.evaluate import PointLogitStore, confusion_matrix, iou_from_confusion
from wsss3d.synthetic import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pseudo_labels.npz")
THRESHOLDS = (0.5, 0.6, 0.7)


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    assert tuple(z["thresholds"]) == THRESHOLDS
    return {k: z[k] for k in z.files}


def _rows_to_scene(offsets, n):
    off = torch.as_tensor(offsets, dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(len(off) - 1), off[1:] - off[:-1], output_size=n)


def _near(top1, top2, masked_f32, thr):
    srt = masked_f32.sort(dim=1)[0]
    tie = srt[:, -1] == srt[:, -2] if masked_f32.size(1) > 1 else torch.zeros(len(top1), dtype=torch.bool)
    return ((top1 - top2 < 1e-6) & ~tie) | (((top1 - thr).abs() < 1e-6) & (top1 != 0.5))


def _restate(logits, scene, offsets, thr):
    """utils/stats.py:5-42 in fp64 on the CPU -> (labels, near rows); non-finite rows -> -100 (the documented
    deviation)."""
    n, c = logits.shape
    if n == 0:
        return torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.bool)
    rows = _rows_to_scene(offsets, n)
    m32 = logits * scene[rows]
    m = logits.double() * scene[rows].double()
    conf = torch.sigmoid(m / m.norm(dim=1, keepdim=True).clamp_min(1e-12))
    top = conf.topk(min(2, c), dim=1)[0]
    top1, top2 = top[:, 0], top[:, -1] if c > 1 else torch.full((n,), -1.0, dtype=torch.float64)
    labels = conf.max(dim=1)[1]
    labels[top1 < thr] = -100
    finite = torch.isfinite(logits).all(1)
    labels[~finite] = -100
    return labels, _near(top1, top2, m32, thr) & finite


def _check_counts(labels, gt, counts, confusion, n_rows, n_classes):
    labels, gt = labels.cpu(), None if gt is None else gt.cpu()
    mask = labels != -100
    exp = [int(mask.sum()), 0 if gt is None else int(((labels == gt) & mask).sum()), n_rows]
    assert counts.cpu().tolist() == exp
    if confusion is not None:
        k = mask & (gt >= 0)
        ref = torch.bincount(labels[k] * n_classes + gt[k], minlength=n_classes ** 2).view(n_classes, n_classes)
        assert torch.equal(confusion.cpu(), ref)


@pytest.mark.parametrize("k", range(3))
def test_fixture_parity(gold, k):
    thr = THRESHOLDS[k]
    logits = torch.from_numpy(gold["logits"])
    scene = torch.from_numpy(gold["scene_label"])
    offsets = gold["batch_offsets"].tolist()
    n = len(logits)
    dl = logits.to(DEV)
    before = dl.clone()
    labels, num = get_pseudo_labels(dl, scene.to(DEV), offsets, thr)
    assert torch.equal(dl, before), "the input logits were modified"
    assert labels.dtype == torch.int64 and labels.shape == (n,) and num.dim() == 0 and num.is_cuda
    near = _near(torch.from_numpy(gold["top1_f64"]), torch.from_numpy(gold["top2_f64"]),
                 logits * scene[_rows_to_scene(offsets, n)], thr)
    print(f"threshold {thr}: near rows {int(near.sum())} / {n}")
    assert int(near.sum()) <= 0.005 * n
    ref = torch.from_numpy(gold[f"labels_{k}"])
    bad = (labels.cpu() != ref) & ~near
    assert not bad.any(), (bad.nonzero().flatten()[:10].tolist(), labels.cpu()[bad][:10], ref[bad][:10])
    assert abs(int(num) - int(gold[f"num_{k}"])) <= int(near.sum())
    assert int(num) == int((labels != -100).sum())
    correct, total = assess_label_quality(labels, torch.from_numpy(gold["gt"]).to(DEV))
    assert int(total) == int(num)
    if not near.any():
        assert [int(correct), int(total)] == gold[f"quality_{k}"].tolist()
    # the same through a tensor of offsets and the accumulating pass (counts, confusion, unchanged input)
    gt = torch.from_numpy(gold["gt"]).to(DEV)
    run = PseudoLabelPass(DEV, threshold=thr)
    l2 = run.add(dl, scene.to(DEV), torch.tensor(offsets, device=DEV), gt)
    assert torch.equal(l2, labels) and torch.equal(dl, before)
    _check_counts(l2, gt, run.counts, run.confusion, n, 20)
    s = run.summary()
    assert s["labelled"] == int(num) and s["correct"] == int(correct) and s["rows"] == n
    assert s["labelled_share"] == int(num) / n and s["precision"] == int(correct) / int(num)
    assert len(s["class_precision"]) == 20


def _case(n, c, b_scenes, seed):
    g = torch.Generator().manual_seed(seed)
    logits = 3 * torch.randn(n, c, generator=g)
    if b_scenes == 1:
        offsets = [0, n]
    else:  # five scenes, two of them empty, one of those last
        cut = sorted(torch.randint(0, n + 1, (2,), generator=g).tolist())
        offsets = [0, cut[0], cut[0], cut[1], n, n]
    scene = (torch.rand(len(offsets) - 1, c, generator=g) < 0.5).float()
    scene[0] = 1.0
    gt = torch.randint(0, c, (n,), generator=g)
    gt[torch.rand(n, generator=g) < 0.2] = -100
    if n > 2:
        logits[1] = -logits[1].abs() - 0.1  # all negative
        logits[2] = 0.0
    return logits, scene, offsets, gt


@pytest.mark.parametrize("c", [1, 7, 20, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_shapes_against_fp64_restatement(n, c):
    """Tile edges (one wave, one 128- or 256-row tile and one row more), every class count the staging treats
    differently (C = 1: no division; odd; the reference's 20; the 64 limit with the 128-row tile), one scene and
    five scenes with two empty ones, with and without gt, accumulated over two calls."""
    for b_scenes in (1, 5):
        logits, scene, offsets, gt = _case(n, c, b_scenes, seed=1000 * n + 10 * c + b_scenes)
        thr = 0.5 if c == 1 else 0.6
        ref, near = _restate(logits, scene, offsets, thr)
        assert int(near.sum()) <= 0.005 * n
        dl, ds, dgt = logits.to(DEV), scene.to(DEV), gt.to(DEV)
        off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
        counts = torch.zeros(3, dtype=torch.int64, device=DEV)
        confusion = torch.zeros((c, c), dtype=torch.int64, device=DEV)
        labels, conf, _ = ops.pseudo_labels(dl, ds, off, thr, gt=dgt, counts=counts, confusion=confusion,
                                            want_conf=True)
        assert torch.equal(dl.cpu(), logits)
        bad = (labels.cpu() != ref) & ~near
        assert not bad.any(), (n, c, b_scenes, bad.nonzero().flatten()[:10].tolist())
        _check_counts(labels, dgt, counts, confusion, n, c)
        if n:
            lab = labels.cpu() != -100
            assert (conf.cpu()[lab] >= thr).all() and (conf.cpu()[~lab] < thr).all()
        # a second call without gt accumulates labelled and rows only
        labels2, _, _ = ops.pseudo_labels(dl, ds, off, thr, counts=counts)
        assert torch.equal(labels2, labels)
        m = int((labels != -100).sum())
        assert counts.cpu().tolist()[0] == 2 * m and counts.cpu().tolist()[2] == 2 * n


def test_non_finite_row_is_unlabelled_and_uncounted():
    logits, scene, offsets, gt = _case(257, 20, 5, seed=5)
    logits[7, 3] = float("nan")
    logits[200, 0] = float("inf")
    scene[:, 3] = 0.0  # the NaN sits in a masked-out class: still non-finite
    ref, near = _restate(logits, scene, offsets, 0.5)
    assert ref[7] == -100 and ref[200] == -100 and not near.any()
    counts = torch.zeros(3, dtype=torch.int64, device=DEV)
    confusion = torch.zeros((20, 20), dtype=torch.int64, device=DEV)
    labels, conf, _ = ops.pseudo_labels(logits.to(DEV), scene.to(DEV), torch.tensor(offsets, device=DEV), 0.5,
                                        gt=gt.to(DEV), counts=counts, confusion=confusion, want_conf=True)
    assert torch.equal(labels.cpu(), ref)
    assert torch.isnan(conf[7]) and torch.isnan(conf[200])
    assert counts.cpu().tolist()[0] == 255  # threshold 0.5 labels every finite row
    _check_counts(labels, gt, counts, confusion, 257, 20)


def test_confusion_accumulates_and_equals_bincount():
    g = torch.Generator().manual_seed(9)
    n = 100000
    pred = torch.randint(0, 20, (n,), generator=g)
    gt = torch.randint(0, 20, (n,), generator=g)
    gt[torch.rand(n, generator=g) < 0.15] = -100
    pred[::1001] = 20   # out of range: skipped
    pred[5::1003] = -100
    conf = None
    for part in (slice(0, 37777), slice(37777, n)):
        conf = confusion_matrix(pred[part].to(DEV), gt[part].to(DEV), out=conf)
    k = (gt >= 0) & (pred >= 0) & (pred < 20)
    ref = torch.bincount(pred[k] * 20 + gt[k], minlength=400).view(20, 20)
    assert conf.dtype == torch.int64 and torch.equal(conf.cpu(), ref)


def test_logit_store_evaluate_matches_the_reference(gold):
    pred, gt = torch.from_numpy(gold["pred"]), torch.from_numpy(gold["gt"])
    assert torch.equal(confusion_matrix(pred.to(DEV), gt.to(DEV)).cpu(), torch.from_numpy(gold["confusion"]))
    store = PointLogitStore(len(pred), DEV)
    store.add(torch.arange(len(pred), device=DEV), F.one_hot(pred, 20).float().to(DEV))
    mean_iou, ious = store.evaluate(gt.to(DEV), return_classes=True)
    assert abs(mean_iou - float(gold["mean_iou"])) <= 1e-12
    assert np.array_equal(ious, iou_from_confusion(gold["confusion"])[0])


def _ce(logits, labels):
    x = logits.clone().requires_grad_(True)
    loss, n_kept, n_bad = point_cross_entropy(x, labels, return_counts=True)
    loss.backward()
    return loss.detach(), x.grad, int(n_kept), int(n_bad)


@pytest.mark.parametrize("n", [1, 65, 2800])
def test_point_ce_against_fp64_fixture(gold, n):
    """Loss within 1e-5 max(1, |ref|) and gradient within 1e-5 max|ref grad| of fp64 (tests/test_gpu_heads.py's
    bars).  n = 2800 is the fixture's own loss and gradient; the prefixes are the same fp64 formula on the
    fixture's first n rows (one row; one tile of 64 and one row more)."""
    logits, gt = torch.from_numpy(gold["logits"])[:n], torch.from_numpy(gold["gt"])[:n].clone()
    if n == 1:
        gt[0] = 4
    if n == 2800:
        ref_loss, ref_grad = float(gold["ce_loss_f64"]), torch.from_numpy(gold["ce_grad"]).double()
    else:
        x = logits.double().requires_grad_(True)
        keep = gt != -100
        ref = F.cross_entropy(x[keep], gt[keep])
        ref.backward()
        ref_loss, ref_grad = ref.item(), x.grad
    loss, grad, n_kept, n_bad = _ce(logits.to(DEV), gt.to(DEV))
    assert n_kept == int((gt != -100).sum()) and n_bad == 0
    print(f"n={n}: loss {loss.item():.8f} ref {ref_loss:.8f}, max grad err "
          f"{(grad.cpu().double() - ref_grad).abs().max().item():.3e} of {ref_grad.abs().max().item():.3e}")
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    assert (grad.cpu().double() - ref_grad).abs().max().item() <= 1e-5 * ref_grad.abs().max().item()
    assert (grad[(gt == -100).to(DEV)] == 0).all()
    loss2, grad2, _, _ = _ce(logits.to(DEV), gt.to(DEV))
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_point_ce_ignored_and_bad_labels(gold):
    logits = torch.from_numpy(gold["logits"])[:300].to(DEV)
    gt = torch.from_numpy(gold["gt"])[:300].clone()
    loss, grad, n_kept, n_bad = _ce(logits, torch.full((300,), -100, dtype=torch.int64, device=DEV))
    assert torch.isnan(loss) and n_kept == 0 and n_bad == 0 and (grad == 0).all()
    gt[3], gt[11], gt[12] = 20, -5, -100
    loss, grad, n_kept, n_bad = _ce(logits, gt.to(DEV))
    ok = (gt >= 0) & (gt < 20)
    assert n_bad == 2 and n_kept == int(ok.sum())
    ref = F.cross_entropy(logits.cpu().double()[ok], gt[ok])
    assert torch.isfinite(loss) and abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    assert (grad[(~ok).to(DEV)] == 0).all() and torch.isfinite(grad).all()


def test_point_ce_step_is_capturable(gold):
    """Forward + backward captured once on static buffers (one stream, no parallel branches); replayed on labels
    with a different number of -100s, loss and gradient are bit-equal to the eager call on those labels."""
    logits = torch.from_numpy(gold["logits"]).to(DEV)
    gt_a = torch.from_numpy(gold["gt"]).to(DEV)
    gt_b = gt_a.clone()
    gt_b[::3] = -100
    assert int((gt_a == -100).sum()) != int((gt_b == -100).sum())
    x = logits.clone().requires_grad_(True)
    y = gt_a.clone()

    def body():
        loss = LOSS_REGISTRY.get("PointClassification")[0](x, y)
        (grad,) = torch.autograd.grad(loss, x)
        return loss, grad

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        body()  # warm-up outside the capture
    g, (loss, grad) = graphs.capture(body, stream)
    torch.cuda.current_stream().wait_stream(stream)
    for labels in (gt_b, gt_a):
        y.copy_(labels)
        g.replay()
        torch.cuda.synchronize()
        e_loss, e_grad, _, _ = _ce(logits, labels)
        assert torch.equal(loss, e_loss) and torch.equal(grad, e_grad)


def test_pseudo_label_training_step_end_to_end():
    """FullySupervised eval logits -> get_pseudo_labels at 0.6 -> one training step on them with
    PointClassification; every parameter gradient within 1e-4 scale + 1e-9 of the same step with
    Classification (test_fused_eval_logits_match_per_point_head's bar)."""
    torch.manual_seed(1)
    b = make_batch(2, 20, seed=6, spacing=0.04)
    pc = EasyDict(name="SparseConvUNet", m=16, dimension=3, full_scale=4096, block_reps=1, residual_blocks=True)
    model = MODEL_REGISTRY.get("FullySupervised")[0](pc).to(DEV)
    with torch.no_grad():
        model.linear.bias.uniform_(-0.5, 0.5)
    x = EasyDict(coords=torch.from_numpy(b["coords"]).to(DEV), feature=torch.from_numpy(b["feats"]).to(DEV),
                 batch_offsets=b["batch_offsets"])
    model.eval()
    with torch.no_grad():
        logits = model(x)
    labels, num = get_pseudo_labels(logits, torch.from_numpy(b["scene_labels"]).to(DEV), b["batch_offsets"], 0.6)
    assert int(num) > 0
    model.train()
    grads = []
    for name in ("PointClassification", "Classification"):
        model.zero_grad(set_to_none=True)
        _, point_logits = model((x, None), istrain=True)
        loss = LOSS_REGISTRY.get(name)[0](point_logits, labels)
        loss.backward()
        grads.append((loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}))
    (lf, gf), (lr, gr) = grads
    assert abs(lf - lr) <= 1e-5 * max(1.0, abs(lr))
    for k in gr:
        scale = max(gr[k].abs().max().item(), 1e-12)
        assert (gf[k] - gr[k]).abs().max().item() <= 1e-4 * scale + 1e-9, k
