"""Batch assembly with elastic distortion: the device path with and without it, against the numpy restatement.

    python scripts/elastic_batch_bench.py [--rooms 8] [--scale 50] [--rounds 20] [--inner 5]

Scenes are procedural rooms at the default 2 cm spacing (wsss3d.synthetic.make_room).  Reported, one JSON line:

  (a) train_merge_gpu(elastic=False): ms per batch (device events around `inner` back-to-back calls, median and
      minimum over `rounds` after three warm-up rounds; a call includes its parameter upload and its one host read);
  (b) train_merge_gpu(elastic=True), the same way: it includes drawing the noise grids on the host and their
      upload (`h2d_noise_bytes`); `host_draw_ms` is the drawing alone; (b)/(a);
  (c) wsss3d.elastic.train_merge_elastic on the same scenes: one process, and the scenes spread over a pool of the
      host cores this process may use (forked before the device is opened);

and the device time of one elastic call by kernel (torch.profiler; null when the profiler gives no device events).
"""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-weakly-supervised-semantic-segmentation_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from wsss3d import elastic as E  # noqa: E402
from wsss3d.synthetic import make_room, train_params  # noqa: E402

_SCENES = None


def _one_scene(job):
    idx, scale = job
    a, b, c = _SCENES[idx]
    params = [train_params(scale, 0, idx)]
    ep = [E.sample_elastic_params(E.abs_extrema(a), params[0][0], scale, 0, idx)]
    return E.merge_elastic_host([(a, b, c, None)], params, ep, 4096)["batch_offsets"][-1]


def host_times(scenes, scale, workers, reps=3):
    """Seconds per batch of the numpy restatement: one process, and `workers` forked processes."""
    global _SCENES
    _SCENES = scenes
    single = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref = E.train_merge_elastic(scenes, scale)
        single.append(time.perf_counter() - t0)
    jobs = [(i, scale) for i in range(len(scenes))]
    with mp.get_context("fork").Pool(workers) as pool:
        pool.map(_one_scene, jobs)  # warm-up: workers started, pages touched
        multi = []
        for _ in range(reps):
            t0 = time.perf_counter()
            pool.map(_one_scene, jobs)
            multi.append(time.perf_counter() - t0)
    return ref, min(single), min(multi)


def timed(fn, rounds, inner):
    import torch
    out = []
    for r in range(rounds + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        if r >= 3:
            out.append(a.elapsed_time(b) / inner)
    return out


def kernel_times(fn):
    """Device microseconds of one call by kernel name (template arguments kept), or None."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            dev = getattr(ev, "device_time_total", None)
            if dev is None:
                dev = getattr(ev, "cuda_time_total", 0)
            if dev and ("kernel" in ev.key or "Memcpy" in ev.key or "scan" in ev.key):
                name = ev.key.replace("msp::", "").split("(")[0]
                name = name[5:] if name.startswith("void ") else name
                out[name] = {"calls": ev.count, "us": round(dev, 1)}
        return out or None
    except Exception as e:  # the measurement above stands without the breakdown
        return {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=8)
    ap.add_argument("--scale", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--workers", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()

    scenes = [make_room(i) for i in range(args.rooms)]
    ref, host_1, host_w = host_times(scenes, args.scale, args.workers)  # before the device is opened
    ext = [E.abs_extrema(a) for a, _, _ in scenes]  # cached by the device path
    draw = []
    for _ in range(3):
        t0 = time.perf_counter()
        eps = [E.sample_elastic_params(ext[i], train_params(args.scale, 0, i)[0], args.scale, 0, i)
               for i in range(len(scenes))]
        draw.append(time.perf_counter() - t0)
    noise_bytes = sum(n.nbytes for e in eps for k in ("noise1", "noise2") for n in e[k])

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("elastic_batch_bench: needs a HIP device (a CPU timing says nothing about the kernels)")
    from wsss3d.merge import DeviceScenes, train_merge_gpu

    sc = DeviceScenes(scenes)
    got = train_merge_gpu(sc, args.scale, elastic=True)
    same = (got.x.batch_offsets == ref["batch_offsets"]
            and np.array_equal(got.x.coords.cpu().numpy(), ref["coords"])
            and np.array_equal(got.x.feature.cpu().numpy(), ref["feats"]))
    t = {"plain": timed(lambda: train_merge_gpu(sc, args.scale), args.rounds, args.inner),
         "elastic": timed(lambda: train_merge_gpu(sc, args.scale, elastic=True), args.rounds, args.inner)}
    kern = kernel_times(lambda: train_merge_gpu(sc, args.scale, elastic=True))
    sizes = [len(a) for a, _, _ in scenes]
    a_ms, b_ms = statistics.median(t["plain"]), statistics.median(t["elastic"])
    print(json.dumps({
        "rooms": args.rooms, "points": sum(sizes), "scale": args.scale, "rows_kept": ref["batch_offsets"][-1],
        "device_equals_restatement": bool(same),
        "a_plain_ms_per_batch": {"median": round(a_ms, 3), "min": round(min(t["plain"]), 3),
                                 "max": round(max(t["plain"]), 3), "ns_per_point": round(a_ms * 1e6 / sum(sizes), 3)},
        "b_elastic_ms_per_batch": {"median": round(b_ms, 3), "min": round(min(t["elastic"]), 3),
                                   "max": round(max(t["elastic"]), 3)},
        "b_over_a": round(b_ms / a_ms, 2), "host_draw_ms": round(min(draw) * 1e3, 2),
        "h2d_noise_bytes": noise_bytes,
        "c_numpy_ms_per_batch": {"one_process": round(host_1 * 1e3, 1), "workers": args.workers,
                                 "worker_pool": round(host_w * 1e3, 1)},
        "elastic_call_by_kernel": kern, "rounds": args.rounds, "inner": args.inner}), flush=True)


if __name__ == "__main__":
    main()
