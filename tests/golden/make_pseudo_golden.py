"""Golden fixture for the pseudo-label stage (run where the reference is readable; the fixture is committed, the
reference is not read at test time).  Loads the reference's own `utils/stats.py` and `utils/iou.py` by path
(they import only os / torch / numpy) and records, for one input:

  * the inputs: logits (N, 20) f32, scene_label (4, 20), batch_offsets, gt (N,) with some -100;
  * `stats.get_pseudo_labels` in fp32 at thresholds 0.5 / 0.6 / 0.7 (labels and num) and
    `stats.assess_label_quality`'s (correct, total) of those labels against gt;
  * the fp64 evaluation of the same formula: per row the top-1 and top-2 confidences (not the full matrix);
  * `iou.confusion_matrix` and the mean IoU (`iou.evaluate`) of a random prediction vector against gt;
  * the fp64 `F.cross_entropy(logits[keep], gt[keep])` and its gradient w.r.t. the (N, 20) logits (the
    gradient is computed in fp64 and stored rounded to f32, 6e-8 relative, to keep the file small).

    python tests/golden/make_pseudo_golden.py <path to the reference checkout>
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
ref_root = sys.argv[1]


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref_root, "utils", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


stats, iou = load("stats"), load("iou")

g = torch.Generator().manual_seed(20)
sizes = [700, 1, 799, 1300]
offsets = [0]
for s in sizes:
    offsets.append(offsets[-1] + s)
N, C = offsets[-1], 20
logits = 3 * torch.randn(N, C, generator=g)
logits[5] = 0.0                                   # an all-zero row: every confidence exactly 0.5
logits[100:140] = -logits[100:140].abs() - 0.1    # all-negative rows: the maximum is an absent class's 0.5
logits[40, 3] = logits[40, 7] = logits[40].max() + 1.0  # an exact tie of the maximum in a scene that may mask it
logits[1000, 2] = logits[1000, 11] = logits[1000].max() + 1.0  # ... and in the all-one scene: first index wins
scene = torch.zeros(4, C)
scene[0] = (torch.rand(C, generator=g) < 0.3).float()
scene[2] = 1.0
scene[3] = (torch.rand(C, generator=g) < 0.5).float()
gt = torch.randint(0, C, (N,), generator=g)
gt[torch.rand(N, generator=g) < 0.1] = -100
pred = torch.randint(0, C, (N,), generator=g)

out = {"logits": logits.numpy(), "scene_label": scene.numpy(), "batch_offsets": np.asarray(offsets, np.int64),
       "gt": gt.numpy(), "pred": pred.numpy(), "thresholds": np.asarray([0.5, 0.6, 0.7])}
for k, thr in enumerate([0.5, 0.6, 0.7]):
    labels, num = stats.get_pseudo_labels(logits.clone(), scene, offsets, thr)  # the reference writes its input
    correct, total = stats.assess_label_quality(labels, gt)
    out[f"labels_{k}"] = labels.numpy()
    out[f"num_{k}"] = np.int64(num.item())
    out[f"quality_{k}"] = np.asarray([correct.item(), total.item()], np.int64)
    print(f"threshold {thr}: labelled {num.item()} / {N}, correct {correct.item()}")

conf64 = stats.preprocess_logits(logits.double(), scene.double(), offsets)
top2 = conf64.topk(2, dim=1)[0]
out["top1_f64"], out["top2_f64"] = top2[:, 0].numpy(), top2[:, 1].numpy()

out["confusion"] = iou.confusion_matrix(pred.numpy(), gt.numpy()).astype(np.int64)
with contextlib.redirect_stdout(io.StringIO()):
    out["mean_iou"] = np.float64(iou.evaluate(pred.numpy(), gt.numpy()))

x = logits.double().requires_grad_(True)
keep = gt != -100
loss = F.cross_entropy(x[keep], gt[keep])
loss.backward()
out["ce_loss_f64"], out["ce_grad"] = np.float64(loss.item()), x.grad.numpy().astype(np.float32)

here = os.path.dirname(os.path.abspath(__file__))
path = os.path.join(here, "pseudo_labels.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes; mean IoU", out["mean_iou"], "CE", out["ce_loss_f64"])
