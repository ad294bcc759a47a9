"""wsss3d.optim.Adam without a device: the header declares the device-hyper-parameter entry point, and the state dict
has torch.optim.Adam's key layout for the same parameter list.

The class steps only on a HIP device (there is no CPU path), so the layout is checked through what builds it, with no
step taken: the constructor's parameter groups (``state_dict()["param_groups"]``) and the helper that lays out one
parameter's state (``_state_layout``), both against a torch.optim.Adam that has taken one CPU step."""
import os
import re

import torch

import __graft_entry__ as g_

g_.add_path()
from wsss3d import optim  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_adam_step_dev():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi3dsparse.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+msp_adam_step_dev\s*\(([^)]*)\)\s*;", src)
    assert m, "include/mi3dsparse.h does not declare msp_adam_step_dev"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const msp_adam_tensor* table", "const int64_t* chunk_start", "const float* const* grads", "int n",
                    "int64_t n_chunks", "float* steps", "const double* hyper", "msp_stream_t stream"]


def _params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5)),
            torch.nn.Parameter(torch.randn(2, 2))]


def test_state_dict_layout_is_torchs():
    ps, pt = _params(), _params()
    groups = lambda q: [{"params": q[:2]}, {"params": q[2:], "lr": 3e-4, "weight_decay": 0.01}]  # noqa: E731
    ours = optim.Adam(groups(ps), lr=1e-3)
    ref = torch.optim.Adam(groups(pt), lr=1e-3)
    for p in pt:
        p.grad = torch.ones_like(p)
    ref.step()
    sd, rd = ours.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rd.keys())
    assert len(sd["param_groups"]) == len(rd["param_groups"])
    for a, b in zip(sd["param_groups"], rd["param_groups"]):
        assert list(a.keys()) == list(b.keys())
        assert a["params"] == b["params"]
        for k in ("lr", "betas", "eps", "weight_decay"):
            assert a[k] == b[k]
    # one parameter's state as _build lays it out (CPU tensors stand in for the device ones)
    p = ps[0]
    st = optim._state_layout(torch.zeros(()), torch.zeros_like(p), torch.zeros_like(p))
    rs = rd["state"][0]
    assert list(st.keys()) == list(rs.keys())
    for k in st:
        assert st[k].shape == rs[k].shape and st[k].dtype == rs[k].dtype, k


def test_unbuilt_optimizer_reports_no_step_count_and_syncs_nothing():
    ours = optim.Adam(_params(), lr=1e-3)
    assert ours.step_count is None
    ours.sync_hyperparameters()  # nothing built, nothing to upload, no device touched
    assert ours.state_dict()["state"] == {}
