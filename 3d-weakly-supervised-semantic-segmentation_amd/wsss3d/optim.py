"""The training loop's optimizer on the library: torch.optim.Adam (train.py:39, ``optim.Adam(model.parameters(),
lr=1e-3)``) as one launch per step over every parameter tensor (``msp_adam_step_dev``, csrc/msp_optim.hip).

torch's fused multi-tensor Adam takes 12 launches of ~50 us per step for the headline UNet's 203 tensors (30.1 M
floats); this is one grid over all of them (plus a one-block launch that advances the step counts), HBM-bound on the
840 MB a step must move.  The update per element is within fp32 rounding of torch's fused Adam (amsgrad off),
checked against ``torch.optim.Adam`` in tests/test_gpu_optim.py and tests/test_gpu_optim_schedule.py.

Graph-capturable after one eager step, and a replayed step follows the rest of train.py:39-44,55-92:

* the gradient pointers of the step being captured travel in the kernel arguments;
* every parameter has its own step count on the device (``state[p]["step"]``), advanced only when the parameter had
  a gradient, as torch does (the text branch that some batches skip keeps its own bias correction);
* lr, betas, eps and weight_decay of each parameter group live in five device doubles that the kernel reads.  An
  eager ``step()`` uploads them whenever they changed, so ``StepLR`` (train.py:43) just works; a replay loop says so
  itself, because nothing can be uploaded from inside a graph::

      scheduler.step(); opt.sync_hyperparameters(); graph.replay()

* ``state_dict()`` has torch's layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter), loads into
  ``torch.optim.Adam`` and takes one saved by it, so a checkpointed run resumes with its bias correction."""
import ctypes

import torch

from sparseconvnet import _lib
from sparseconvnet._lib import call, ptr

_MAX_TENSORS = 256  # MSP_ADAM_MAX_TENSORS
_UNSUPPORTED = ("amsgrad", "maximize", "differentiable", "decoupled_weight_decay")


class _Tensor(ctypes.Structure):  # msp_adam_tensor
    _fields_ = [("param", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("n", ctypes.c_int64)]


def _group_defaults(lr, betas, eps, weight_decay):
    """A parameter group's keys: exactly torch.optim.Adam's (whatever the installed torch keeps there), so a state
    dict moves between the two classes.  This class is what torch calls fused and capturable: one device launch,
    step counts on the device; torch's loader reads those two flags to decide where ``step`` lives."""
    d = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
    d.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    for k in ("fused", "capturable"):
        if k in d:
            d[k] = True
    return d


def _state_layout(step, exp_avg, exp_avg_sq):
    """One parameter's state, torch.optim.Adam's keys in torch's order."""
    return {"step": step, "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}


def _hyper(g):
    b1, b2 = g["betas"]
    return (float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]))


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's update (lr, betas, eps, weight_decay; amsgrad and maximize off) on fp32 device
    parameters.  State per parameter as in torch: ``step`` (a 0-dim view into the device array of its launch's
    counts), ``exp_avg`` and ``exp_avg_sq``.  ``step_count`` is the largest count (a 0-dim device tensor; None
    before the first step)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, _group_defaults(lr, betas, eps, weight_decay))
        self._built = None
        self._key = None
        self._device = None
        self._hyper_dev = []  # per group: [device double[5], the values last uploaded]

    @property
    def step_count(self):
        if not self._built:
            return None
        return torch.cat([b[4] for b in self._built]).max()

    def load_state_dict(self, state_dict):
        """A state dict saved by this class or by ``torch.optim.Adam`` over the same parameters (its ``step`` may be
        a CPU tensor or a number).  The next step rebuilds the tables around the loaded state."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:  # whatever the saving optimizer was, this one keeps its counts on the device
            for k in ("fused", "capturable"):
                if k in self.defaults:
                    g[k] = True
        self._built = None

    def _name(self, gi, i):
        names = self.param_groups[gi].get("param_names")
        return f"'{names[i]}'" if names else f"#{i} of group {gi}"

    def _build(self):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("wsss3d.optim.Adam: take one step eagerly before capturing steps in a graph (the first "
                               "step allocates the moments and uploads the tensor table)")
        params = [p for g in self.param_groups for p in g["params"]]
        if not params:
            self._built, self._key = [], ()
            return
        dev = params[0].device
        for gi, g in enumerate(self.param_groups):
            on = [k for k in _UNSUPPORTED if g.get(k)]
            if on:
                raise RuntimeError(f"wsss3d.optim.Adam: group {gi} asks for {', '.join(on)}, which this optimizer "
                                   "does not implement")
            for i, p in enumerate(g["params"]):
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.device == dev):
                    raise RuntimeError("wsss3d.optim.Adam: parameters must be contiguous fp32 tensors on one HIP "
                                       "device")
                st = self.state[p]
                for k in ("exp_avg", "exp_avg_sq"):
                    m = st.get(k)
                    if m is not None and not (torch.is_tensor(m) and m.shape == p.shape and m.dtype == p.dtype
                                              and m.device == p.device and m.is_contiguous()):
                        what = f"{tuple(m.shape)} {m.dtype} on {m.device}" if torch.is_tensor(m) else type(m).__name__
                        raise RuntimeError(f"wsss3d.optim.Adam: state '{k}' of parameter {self._name(gi, i)} "
                                           f"({what}) does not match the parameter ({tuple(p.shape)} {p.dtype} on "
                                           f"{p.device}, contiguous)")
        self._device = dev
        # one table per group of <= MSP_ADAM_MAX_TENSORS tensors, with its step counts; the group's hyper-parameters
        # in a device block that outlives rebuilds
        built = []
        for gi, g in enumerate(self.param_groups):
            if gi == len(self._hyper_dev):
                self._hyper_dev.append([torch.zeros(5, dtype=torch.float64, device=dev), None])
            ps = list(g["params"])
            for k in range(0, len(ps), _MAX_TENSORS):
                part = ps[k:k + _MAX_TENSORS]
                steps = self._gather_steps([self.state[p].get("step") for p in part], dev)
                tab = (_Tensor * len(part))()
                starts = [0]
                for i, p in enumerate(part):
                    st = self.state[p]
                    m = st.pop("exp_avg", None)
                    v = st.pop("exp_avg_sq", None)
                    st.pop("step", None)
                    rest = dict(st)
                    st.clear()
                    st.update(_state_layout(steps[i],
                                            torch.zeros_like(p, memory_format=torch.contiguous_format) if m is None else m,
                                            torch.zeros_like(p, memory_format=torch.contiguous_format) if v is None else v))
                    st.update(rest)
                    tab[i] = _Tensor(p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
                    starts.append(starts[-1] + int(_lib.query("msp_adam_chunks", _lib.I64(p.numel()))))
                dtab = torch.frombuffer(bytearray(tab), dtype=torch.uint8).to(dev)
                dstart = torch.tensor(starts, dtype=torch.int64, device=dev)
                built.append((gi, part, dtab, dstart, steps, starts[-1]))
        self._built = built
        # what the table points at: a parameter moved or re-allocated (model.to(...), load_state_dict into new
        # storage, a group added) means a rebuild, never a write through a stale pointer
        self._key = self._table_key()

    @staticmethod
    def _gather_steps(vals, dev):
        """The counts a rebuilt table starts from: what the state holds (views into the previous array, or a loaded
        state dict's device tensors, CPU tensors or numbers), zero for a parameter without state."""
        steps = torch.zeros(len(vals), dtype=torch.float32, device=dev)
        on_dev = [(i, v) for i, v in enumerate(vals) if torch.is_tensor(v) and v.is_cuda]
        on_host = [(i, float(v)) for i, v in enumerate(vals) if v is not None and not (torch.is_tensor(v) and v.is_cuda)]
        if on_dev:
            idx = torch.tensor([i for i, _ in on_dev], device=dev)
            steps[idx] = torch.stack([v.detach().reshape(()).to(device=dev, dtype=torch.float32) for _, v in on_dev])
        if on_host:
            idx = torch.tensor([i for i, _ in on_host], device=dev)
            steps[idx] = torch.tensor([x for _, x in on_host], dtype=torch.float32).to(dev)
        return steps

    def _table_key(self):
        return tuple((id(p), p.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr())
                     if p in self.state and "exp_avg" in self.state[p] else (id(p), p.data_ptr(), 0, 0)
                     for g in self.param_groups for p in g["params"])

    def sync_hyperparameters(self):
        """Copy every group's (lr, betas, eps, weight_decay) that changed since its last upload into the group's
        device block: one 40-byte copy per changed group on the current stream, nothing when nothing changed.
        ``step()`` does this itself outside capture; a loop that replays a captured step calls it after the
        scheduler and before ``graph.replay()``.  Inside a capture nothing is uploaded (the graph reads the block)."""
        for g, slot in zip(self.param_groups, self._hyper_dev):
            h = _hyper(g)
            if h != slot[1]:
                if torch.cuda.is_current_stream_capturing():
                    return
                slot[0].copy_(torch.tensor(h, dtype=torch.float64))
                slot[1] = h

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._built is None or self._table_key() != self._key:
            self._build()
        if not self._built:
            return loss
        self.sync_hyperparameters()
        stream = _lib.stream(self._device)
        for gi, part, dtab, dstart, steps, n_chunks in self._built:
            grads = []
            for p in part:
                gr = p.grad
                if gr is not None:
                    if gr.dtype != torch.float32 or gr.shape != p.shape:
                        raise RuntimeError("wsss3d.optim.Adam: gradient dtype / shape does not match its parameter")
                    if not gr.is_contiguous():
                        gr = p.grad = gr.contiguous()
                grads.append(gr)
            # an empty gradient has no storage: any non-NULL pointer says "had a gradient" (it is never read)
            arr = (ctypes.c_void_p * len(part))(*[(ptr(gr) or ptr(steps)) if gr is not None else None for gr in grads])
            call("msp_adam_step_dev", ptr(dtab), ptr(dstart), ctypes.cast(arr, ctypes.c_void_p), len(part), n_chunks,
                 ptr(steps), ptr(self._hyper_dev[gi][0]), stream)
        return loss
