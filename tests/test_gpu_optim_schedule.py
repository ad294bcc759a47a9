"""wsss3d.optim.Adam on msp_adam_step_dev (device hyper-parameters, one step count per parameter) against
torch.optim.Adam fed the same gradients: a StepLR schedule followed by a replayed graph, a parameter that only sometimes
gets a gradient, the sizes around the kernel's chunk with more tensors than one launch takes, the state dict in both
directions, determinism, and the guard on a mis-sized moment.

Tolerances are those of tests/test_gpu_optim.py for the same comparison: parameters rtol 2e-6 / atol 2e-7, moments
rtol 1e-6 / atol 1e-7 (O(1) gradients, one fp32 rounding of torch's own expression order)."""
import copy
import functools

import pytest
import torch

import __graft_entry__ as g_

g_.add_path()
from sparseconvnet import _lib  # noqa: E402
from wsss3d.optim import Adam  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
P_TOL = dict(rtol=2e-6, atol=2e-7)
M_TOL = dict(rtol=1e-6, atol=1e-7)


def _params(shapes, seed):
    torch.manual_seed(seed)
    return [torch.randn(*s, device=DEV) for s in shapes]


def _make(cls, init, groups, **kw):
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    return ps, cls([{"params": [ps[i] for i in idx], **extra} for idx, extra in groups], **kw)


def _set_grads(ps, grads):
    for p, gr in zip(ps, grads):
        p.grad = None if gr is None else gr.clone()


def _assert_matches(ours, ps_o, ref, ps_r, steps=False):
    for a, b in zip(ps_o, ps_r):
        torch.testing.assert_close(a.detach(), b.detach(), **P_TOL)
        sa, sb = ours.state.get(a, {}), ref.state.get(b, {})
        if "exp_avg" not in sb:
            continue
        torch.testing.assert_close(sa["exp_avg"], sb["exp_avg"], **M_TOL)
        torch.testing.assert_close(sa["exp_avg_sq"], sb["exp_avg_sq"], **M_TOL)
        if steps:
            assert float(sa["step"]) == float(sb["step"])


def _assert_bitwise(opt_a, ps_a, opt_b, ps_b):
    for a, b in zip(ps_a, ps_b):
        assert torch.equal(a.detach(), b.detach())
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[a][k], opt_b.state[b][k]), k


def test_schedule_under_replay():
    """train.py:39-44 under replay: Adam + StepLR, the step captured once and replayed after
    ``scheduler.step(); sync_hyperparameters()``.  Every step matches torch eager under the same scheduler, and is
    bitwise what this optimizer does eagerly; with the lr left constant the third step is different."""
    init = _params([(128, 96), (96,), (5, 3), (2049,)], 11)
    groups = [([0, 1], {}), ([2, 3], {"lr": 3e-4})]
    grads = [[torch.randn_like(t) for t in init] for _ in range(7)]
    sched = lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=2, gamma=0.5)  # noqa: E731
    ps_g, opt_g = _make(Adam, init, groups, lr=1e-3)  # replayed
    ps_e, opt_e = _make(Adam, init, groups, lr=1e-3)  # eager, same scheduler
    ps_c, opt_c = _make(Adam, init, groups, lr=1e-3)  # eager, constant lr (the control)
    ps_t, opt_t = _make(torch.optim.Adam, init, groups, lr=1e-3, fused=True)
    sch_g, sch_e, sch_t = sched(opt_g), sched(opt_e), sched(opt_t)
    for ps, opt in ((ps_g, opt_g), (ps_e, opt_e), (ps_c, opt_c), (ps_t, opt_t)):
        _set_grads(ps, grads[0])
        opt.step()  # the eager first step: moments, tables
    _assert_matches(opt_g, ps_g, opt_t, ps_t, steps=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        graph.capture_begin()
        opt_g.step()
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    for k in range(1, 7):
        for p, gr in zip(ps_g, grads[k]):
            p.grad.copy_(gr)  # the captured launch keeps these buffers' pointers
        sch_g.step()
        opt_g.sync_hyperparameters()
        graph.replay()
        for ps, opt, sch in ((ps_e, opt_e, sch_e), (ps_t, opt_t, sch_t)):
            sch.step()
            _set_grads(ps, grads[k])
            opt.step()
        _assert_matches(opt_g, ps_g, opt_t, ps_t, steps=True)
        _assert_bitwise(opt_g, ps_g, opt_e, ps_e)
        if k <= 2:
            _set_grads(ps_c, grads[k])
            opt_c.step()
        if k == 1:  # lr not yet changed: the control is still the same run
            _assert_bitwise(opt_g, ps_g, opt_c, ps_c)
        if k == 2:  # third step, the first at half the lr
            assert opt_g.param_groups[0]["lr"] == 5e-4 and opt_c.param_groups[0]["lr"] == 1e-3
            for a, b in zip(ps_g, ps_c):
                assert not torch.allclose(a.detach(), b.detach(), **P_TOL)
    assert float(opt_g.step_count) == 7.0


def test_intermittent_gradients_keep_their_own_step():
    """A parameter without a gradient on steps 2 and 3 of 5 (the text branch of a batch with no text): its step count
    stays behind, so its bias correction is torch's."""
    init = _params([(64, 48), (300,), (7,), (2048 * 2 + 5,)], 12)
    groups = [([0, 1, 2, 3], {})]
    ps_o, ours = _make(Adam, init, groups, lr=1e-3)
    ps_t, ref = _make(torch.optim.Adam, init, groups, lr=1e-3, fused=True)
    for k in range(1, 6):
        grads = [torch.randn_like(t) for t in init]
        if k in (2, 3):
            grads[1] = None
        _set_grads(ps_o, grads)
        _set_grads(ps_t, grads)
        ours.step()
        ref.step()
        _assert_matches(ours, ps_o, ref, ps_t, steps=True)
    assert [float(ours.state[p]["step"]) for p in ps_o] == [5.0, 3.0, 5.0, 5.0]
    assert all(ours.state[p]["step"].dim() == 0 and ours.state[p]["step"].is_cuda for p in ps_o)


def _chunk():
    """Floats per block of the step kernel, from msp_adam_chunks."""
    chunks = _lib.load().msp_adam_chunks
    c = 1
    while chunks(c + 1) == 1:
        c += 1
    assert chunks(c) == 1 and chunks(c + 1) == 2 and chunks(3 * c + 1) == 4
    return c


def _shape_case():
    c = _chunk()
    sizes = [1, 7, c, c - 1, c + 1, 3 * c + 1, 2 * c + 4]  # the last: the float4 path with a part-filled last chunk
    shapes = [(sizes[i % len(sizes)],) for i in range(257)]  # > MSP_ADAM_MAX_TENSORS: a second table
    init = _params(shapes, 13)
    grads = [[torch.randn_like(t) for t in init] for _ in range(3)]
    return init, grads


def _shape_run(cls, wd, **kw):
    init, grads = _shape_case()
    ps, opt = _make(cls, init, [(list(range(len(init))), {})], lr=1e-3, weight_decay=wd, **kw)
    for sg in grads:
        _set_grads(ps, sg)
        opt.step()
    torch.cuda.synchronize()
    return ps, opt


_ours_shape_run = functools.lru_cache(maxsize=None)(functools.partial(_shape_run, Adam))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_chunk_edge_sizes_and_second_table(wd):
    ps_o, ours = _ours_shape_run(wd)
    ps_t, ref = _shape_run(torch.optim.Adam, wd, fused=True)
    _assert_matches(ours, ps_o, ref, ps_t, steps=True)
    assert all(float(ours.state[p]["step"]) == 3.0 for p in ps_o)
    assert float(ours.step_count) == 3.0


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_deterministic(wd):
    ps_a, opt_a = _ours_shape_run(wd)
    ps_b, opt_b = _shape_run(Adam, wd)
    _assert_bitwise(opt_a, ps_a, opt_b, ps_b)


_RT_SHAPES = [(96, 40), (40,), (2049,), (3, 5)]
_RT_GROUPS = [([0, 1], {}), ([2, 3], {"lr": 3e-4, "weight_decay": 0.01})]


def _round_trip_grads(init):
    torch.manual_seed(14)
    grads = [[torch.randn_like(t) for t in init] for _ in range(4)]
    grads[1][1] = None  # counts differ between parameters, so a resumed run needs each of them
    return grads


def _steps(ps, opt, grads):
    for sg in grads:
        _set_grads(ps, sg)
        opt.step()


def _resume(cls, ps_from, state_dict, **kw):
    ps, opt = _make(cls, [p.detach() for p in ps_from], _RT_GROUPS, lr=1e-3, **kw)
    opt.load_state_dict(state_dict)
    return ps, opt


def test_state_dict_resumes_bitwise():
    init = _params(_RT_SHAPES, 15)
    grads = _round_trip_grads(init)
    ps_a, opt_a = _make(Adam, init, _RT_GROUPS, lr=1e-3)
    _steps(ps_a, opt_a, grads)  # uninterrupted
    ps_b, opt_b = _make(Adam, init, _RT_GROUPS, lr=1e-3)
    _steps(ps_b, opt_b, grads[:3])
    saved = copy.deepcopy(opt_b.state_dict())  # as a checkpoint written and read back
    assert [float(saved["state"][i]["step"]) for i in range(4)] == [3.0, 2.0, 3.0, 3.0]
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in saved["state"].values())
    ps_c, opt_c = _resume(Adam, ps_b, saved)
    _steps(ps_c, opt_c, grads[3:])
    _assert_bitwise(opt_a, ps_a, opt_c, ps_c)


@pytest.mark.parametrize("step_as", ["device_tensor", "cpu_tensor", "number"])
def test_loads_a_torch_adam_state_dict(step_as):
    init = _params(_RT_SHAPES, 16)
    grads = _round_trip_grads(init)
    ps_t, ref = _make(torch.optim.Adam, init, _RT_GROUPS, lr=1e-3, fused=True)
    _steps(ps_t, ref, grads[:3])
    saved = copy.deepcopy(ref.state_dict())
    for st in saved["state"].values():
        if step_as == "cpu_tensor":
            st["step"] = st["step"].cpu()
        elif step_as == "number":
            st["step"] = float(st["step"])
    if step_as != "device_tensor":  # what a torch.optim.Adam that keeps its counts on the host writes
        for g in saved["param_groups"]:
            g["fused"], g["capturable"] = None, False
    ps_o, ours = _resume(Adam, ps_t, saved)
    _steps(ps_o, ours, grads[3:])
    _steps(ps_t, ref, grads[3:])
    _assert_matches(ours, ps_o, ref, ps_t, steps=True)
    assert [float(ours.state[p]["step"]) for p in ps_o] == [4.0, 3.0, 4.0, 4.0]


def test_state_dict_loads_into_torch_adam():
    init = _params(_RT_SHAPES, 17)
    grads = _round_trip_grads(init)
    ps_o, ours = _make(Adam, init, _RT_GROUPS, lr=1e-3)
    _steps(ps_o, ours, grads[:3])
    saved = copy.deepcopy(ours.state_dict())
    ps_t, ref = _resume(torch.optim.Adam, ps_o, saved, fused=True)
    _steps(ps_t, ref, grads[3:])
    _steps(ps_o, ours, grads[3:])
    _assert_matches(ours, ps_o, ref, ps_t, steps=True)


def test_build_rejects_a_mis_sized_moment():
    init = _params([(33, 17), (64,)], 18)
    ps, opt = _make(Adam, init, [([0, 1], {})], lr=1e-3)
    _set_grads(ps, [torch.randn_like(t) for t in init])
    opt.step()
    before = [p.detach().clone() for p in ps]
    opt.state[ps[1]]["exp_avg"] = torch.zeros(ps[1].numel() - 1, device=DEV)
    with pytest.raises(RuntimeError, match=r"exp_avg.*parameter #1 of group 0"):
        opt.step()
    torch.cuda.synchronize()
    for p, b in zip(ps, before):  # nothing was launched
        assert torch.equal(p.detach(), b)
    assert [float(opt.state[p]["step"]) for p in ps] == [1.0, 1.0]
