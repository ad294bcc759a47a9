"""Golden fixture for the drop-in check (run where a checkout of the reference is readable; the fixture is
committed, the reference is not read at test time).  Loads the reference's own `models/SparseConvNet.py`
unmodified, with THIS package as `sparseconvnet`, builds its encoders at a fixed seed and records, per encoder,
every state_dict entry's key, shape, leading values and sums, plus the names the file takes from the
`sparseconvnet` namespace.

    python tests/golden/make_dropin_golden.py <path of the reference checkout>
"""
import ast
import importlib.util
import json
import os
import sys
import types

import torch

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
for p in (os.path.join(root, "3d-weakly-supervised-semantic-segmentation_amd"), root):
    if p not in sys.path:
        sys.path.insert(0, p)

import sparseconvnet as scn  # noqa: E402
from wsss3d import EasyDict  # noqa: E402

SEED, HEAD = 5, 32
CONFIGS = [("SparseConvUNet", 32, 2, True), ("SparseConvFCNet", 16, 1, False),
           ("SparseConvFCNetDirectUpPoolLight", 16, 1, True)]

ref_root = sys.argv[1]
path = os.path.join(ref_root, "models", "SparseConvNet.py")
sys.modules["easydict"] = types.SimpleNamespace(EasyDict=EasyDict)
if ref_root not in sys.path:
    sys.path.append(ref_root)
spec = importlib.util.spec_from_file_location("ref_models_on_mi3dsparse", path)
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
assert mod.scn is scn

with open(path) as f:
    tree = ast.parse(f.read())
names = sorted({n.attr for n in ast.walk(tree)
                if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "scn"})

out = {"seed": SEED, "head": HEAD, "scn_names": names, "encoders": {}}
for name, m, reps, res in CONFIGS:
    torch.manual_seed(SEED)
    enc = getattr(mod, name)(name, m=m, dimension=3, full_scale=4096, block_reps=reps, residual_blocks=res)
    out["encoders"][f"{name}-m{m}-r{reps}-{int(res)}"] = [
        [k, list(v.shape), v.reshape(-1)[:HEAD].double().tolist(), v.double().sum().item(),
         v.double().abs().sum().item()] for k, v in enc.state_dict().items()]
with open(os.path.join(here, "dropin_state.json"), "w") as f:
    json.dump(out, f)
print("wrote dropin_state.json", {k: len(v) for k, v in out["encoders"].items()}, names)
