"""Device time of one Adam step over the headline UNet's parameters: msp_adam_step (host hyper-parameters, one
shared step count) against msp_adam_step_dev (device hyper-parameters, one count per tensor), same tensors, same
gradients.

The parameter list is the headline model's (MultiLabel over SparseConvUNet m=32, two blocks per level, residual:
203 tensors, 30.1 M floats; a step reads param, grad and both moments and writes three of them, 840 MB).  Three arms
run interleaved in one process, each call between two device events, after a warm-up: the old entry, the new one, and
the old entry again.  The two old arms are the same code, so the gap between their medians is the margin below which
a difference says nothing.  Prints per arm the median and the minimum in microseconds, and the algorithmic GB/s at the
median; --out also writes the report to a file.

Usage: python scripts/adam_step_bench.py [--rounds 40] [--warmup 10] [--out profiles/optim/adam_step_bench.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import __graft_entry__ as g_  # noqa: E402

g_.add_path()
import torch  # noqa: E402

from sparseconvnet import _lib  # noqa: E402
from sparseconvnet._lib import call, ptr  # noqa: E402
from wsss3d import EasyDict, MODEL_REGISTRY  # noqa: E402
from wsss3d.optim import _Tensor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.rounds < 20:
    sys.exit("adam_step_bench: at least 20 rounds")
if not torch.cuda.is_available():
    sys.exit("adam_step_bench: needs a HIP device (a timing taken anywhere else says nothing)")

_lib.load()
dev = torch.device("cuda:0")
torch.manual_seed(0)
pc = EasyDict(name="SparseConvUNet", m=32, dimension=3, full_scale=4096, block_reps=2, residual_blocks=True)
cls, _ = MODEL_REGISTRY.get("MultiLabel")
params = [p.detach().clone() for p in cls(pc).to(dev).parameters()]
n_floats = sum(p.numel() for p in params)

LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.0
tables = []
for k in range(0, len(params), 256):  # MSP_ADAM_MAX_TENSORS per launch
    part = params[k:k + 256]
    grads = [torch.randn_like(p) for p in part]
    m, v = [torch.zeros_like(p) for p in part], [torch.zeros_like(p) for p in part]
    tab = (_Tensor * len(part))()
    starts = [0]
    for i, p in enumerate(part):
        tab[i] = _Tensor(p.data_ptr(), m[i].data_ptr(), v[i].data_ptr(), p.numel())
        starts.append(starts[-1] + int(_lib.query("msp_adam_chunks", _lib.I64(p.numel()))))
    tables.append(dict(
        n=len(part), n_chunks=starts[-1], keep=(grads, m, v),
        tab=torch.frombuffer(bytearray(tab), dtype=torch.uint8).to(dev),
        start=torch.tensor(starts, dtype=torch.int64, device=dev),
        grads=(ctypes.c_void_p * len(part))(*[ptr(g) for g in grads]),
        steps=torch.zeros(len(part), dtype=torch.float32, device=dev)))
step = torch.zeros(1, dtype=torch.float32, device=dev)
hyper = torch.tensor([LR, B1, B2, EPS, WD], dtype=torch.float64, device=dev)
stream = _lib.stream(dev)


def old():
    for j, t in enumerate(tables):
        call("msp_adam_step", ptr(t["tab"]), ptr(t["start"]), ctypes.cast(t["grads"], ctypes.c_void_p), t["n"],
             t["n_chunks"], ptr(step), int(j == 0), LR, B1, B2, EPS, WD, stream)


def new():
    for t in tables:
        call("msp_adam_step_dev", ptr(t["tab"]), ptr(t["start"]), ctypes.cast(t["grads"], ctypes.c_void_p), t["n"],
             t["n_chunks"], ptr(t["steps"]), ptr(hyper), stream)


ARMS = [("msp_adam_step", old), ("msp_adam_step_dev", new), ("msp_adam_step (again)", old)]
times = [[] for _ in ARMS]
for r in range(args.warmup + args.rounds):
    for a, (_, fn) in enumerate(ARMS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= args.warmup:
            times[a].append(e0.elapsed_time(e1) * 1e3)

gb = 7 * 4 * n_floats / 1e9
lines = [f"adam_step_bench: {len(params)} tensors, {n_floats / 1e6:.1f} M floats, {gb * 1e3:.0f} MB per step; "
         f"{args.rounds} interleaved rounds after {args.warmup} warm-up, device events around each call "
         f"(its second launch included)",
         f"{'arm':<24}{'median us':>12}{'min us':>10}{'GB/s at median':>16}"]
med = []
for (name, _), t in zip(ARMS, times):
    med.append(statistics.median(t))
    lines.append(f"{name:<24}{med[-1]:>12.1f}{min(t):>10.1f}{gb / (med[-1] * 1e-6):>16.0f}")
spread = abs(med[0] - med[2])
delta = med[1] - 0.5 * (med[0] + med[2])
lines.append(f"old entry against itself (the margin): {spread:.1f} us; new - old (mean of the two old medians): "
             f"{delta:+.1f} us -> " + ("inside the margin" if abs(delta) <= spread else
                                       ("slower than the margin" if delta > 0 else "faster than the margin")))
report = "\n".join(lines)
print(report)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(report + "\n")
