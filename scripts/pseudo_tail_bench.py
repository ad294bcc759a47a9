"""Pseudo-label training tail: the per-point tail against the voxel-level tail, from the same level-0 voxel rows.

    python scripts/pseudo_tail_bench.py [--batch 8] [--scale 50] [--m 32] [--rounds 20] [--inner 5]

The headline batch (`make_batch(8, 50, seed=0)`) goes once through SparseConvUNet m=32 up to its OutputLayer; the
rows it leaves (V, m) are detached and both tails start from them:

  point  PointLogitsFunction + segment_mean + point_cross_entropy  (FullySupervised.forward(istrain=True) with
         PointClassification: the (N, 20) logits, their gradient, msp_output_bwd back onto the voxel rows)
  voxel  voxel_point_cross_entropy  (ops.VoxelCrossEntropyFunction: FullySupervised.point_loss)

each forward + backward of `multilabel_soft_margin_loss(scene_logits, y) + point loss` down to the gradients of
the rows, the Linear's weight and its bias.  Labels are the model's own pseudo labels at threshold 0.6.  Timed
with device events around `inner` back-to-back steps, the two tails alternating inside one process, median /
minimum / maximum over `rounds` after three warm-up rounds.  Peak memory is torch's max_memory_allocated above
what is allocated before the step, one step of each tail in a run of its own after the timing.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-weakly-supervised-semantic-segmentation_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fns, rounds, inner):
    """fns: name -> callable.  Alternates the callables; returns name -> list of microseconds per call."""
    out = {k: [] for k in fns}
    for r in range(rounds + 3):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            if r >= 3:  # three warm-up rounds
                out[k].append(a.elapsed_time(b) * 1e3 / inner)
    return out


def peak_above_baseline(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scale", type=float, default=50)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.6)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pseudo_tail_bench: needs a HIP device (a CPU timing says nothing about the kernels)")
    from sparseconvnet.ops import PointLogitsFunction
    from wsss3d import EasyDict, MODEL_REGISTRY, get_pseudo_labels, point_cross_entropy, segment_mean, \
        voxel_point_cross_entropy
    from wsss3d.synthetic import make_batch

    dev = "cuda:0"
    torch.manual_seed(0)
    b = make_batch(args.batch, args.scale, seed=0)
    pc = EasyDict(name="SparseConvUNet", m=args.m, dimension=3, full_scale=4096, block_reps=args.reps,
                  residual_blocks=True)
    model = MODEL_REGISTRY.get("FullySupervised")[0](pc).to(dev)
    coords, feats = torch.from_numpy(b["coords"]).to(dev), torch.from_numpy(b["feats"]).to(dev)
    offsets = b["batch_offsets"]
    y = torch.from_numpy(b["scene_labels"]).to(dev)
    B = len(offsets) - 1
    enc = model.pc_encoder
    with torch.no_grad():
        t = enc.encoder[:-1]([coords, feats])
        rules = t.metadata.input
        if not rules.scene_ranges_match(offsets):
            raise SystemExit("pseudo_tail_bench: the batch's scenes are not its batch ids")
        level = t.metadata.level(int(t.spatial_size[0]))
        rows = t.features.detach().clone()
        logits = PointLogitsFunction.apply(rows, model.linear.weight, model.linear.bias, rules)
        labels, num = get_pseudo_labels(logits, y, offsets, args.threshold)
        del logits, t
    x = rows.requires_grad_(True)
    W, bias = model.linear.weight, model.linear.bias
    N, V = rules.n_points, rows.size(0)

    def point_tail():
        logits = PointLogitsFunction.apply(x, W, bias, rules)
        loss = F.multilabel_soft_margin_loss(segment_mean(logits, offsets), y) + point_cross_entropy(logits, labels)
        return (loss,) + torch.autograd.grad(loss, (x, W, bias))

    def voxel_tail():
        scene, point = voxel_point_cross_entropy(x, W, bias, labels, level, rules, B)
        loss = F.multilabel_soft_margin_loss(scene, y) + point
        return (loss,) + torch.autograd.grad(loss, (x, W, bias))

    # the same results first
    rp, rv = point_tail(), voxel_tail()
    diffs = {"loss_abs_diff": abs(rp[0].item() - rv[0].item())}
    for name, gp, gv in zip(("dx", "dW", "db"), rp[1:], rv[1:]):
        diffs[name + "_rel_diff"] = ((gp - gv).abs().max() / gp.abs().max()).item()
    del rp, rv

    ts = timed({"point": point_tail, "voxel": voxel_tail}, args.rounds, args.inner)
    res = {"points": N, "voxels": V, "scenes": B, "m": args.m, "classes": W.size(0), "labelled": int(num),
           "rounds": args.rounds, "inner": args.inner, "point_logits_bytes": N * W.size(0) * 4, **diffs}
    for k, v in ts.items():
        res[k] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1),
                  "max_us": round(max(v), 1)}
    res["point"]["peak_bytes"] = peak_above_baseline(point_tail)
    res["voxel"]["peak_bytes"] = peak_above_baseline(voxel_tail)
    res["voxel_over_point_time"] = round(res["voxel"]["median_us"] / res["point"]["median_us"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
