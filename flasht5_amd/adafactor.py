"""`Adafactor` on MI355X: the optimizer T5 was trained with, with the arguments, per-group options, state keys and arithmetic of
`transformers.optimization.Adafactor` (a `state_dict` moves between the two classes), its whole step fused into four HIP launches
per (device, parameter dtype, gradient dtype, first moment) bucket of a parameter group through the C ABI (`fat5_adafactor_step`,
csrc/adafactor_kernels.h) instead of some twenty eager launches and two fp32 copies per tensor.  All state and all arithmetic are
fp32 whatever the parameter dtype; the parameter is rounded once, when it is stored."""
import ctypes
import math

import torch
from torch.optim import Optimizer

from . import _lib
from ._captured_step import CapturedStepHost

__all__ = ["Adafactor"]


class _Desc(ctypes.Structure):
    """mirror of `fat5_adafactor_tensor` (include/fat5.h)"""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("vr", ctypes.c_void_p), ("vc", ctypes.c_void_p), ("m", ctypes.c_void_p),
                ("rms", ctypes.c_void_p), ("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("ws_begin", ctypes.c_int64),
                ("tile_begin", ctypes.c_int32), ("fblock_begin", ctypes.c_int32), ("beta2t", ctypes.c_float), ("rho", ctypes.c_float)]


class Adafactor(Optimizer, CapturedStepHost):
    """Same arguments, argument checks and per-group options as `transformers.optimization.Adafactor`; state keys and shapes are its
    own (`step`, `exp_avg_sq_row` (R,) and `exp_avg_sq_col` (C,) for 2-D parameters, `exp_avg_sq` for 1-D ones, `exp_avg` with
    `beta1`, `RMS`), all fp32; `step` is a host integer.

    There is NO CPU fallback: parameters must live on the HIP device.  Raised before any launch: parameters with more than two
    dimensions (HF's batched-matrix case), sparse gradients, non-contiguous parameters or gradients, CPU parameters.

    A step can be recorded into a HIP graph (`GraphedTrainStep`, or by hand: `init_state()`, capture `step()`, then
    `graph_advance()` before every replay): `beta2t`, the relative step (or the group's `lr`, so LR schedulers keep working with
    `relative_step=False`) and `weight_decay` reach the captured launches through device memory."""

    def __init__(self, params, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                 scale_parameter=True, relative_step=True, warmup_init=False):
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if warmup_init and not relative_step:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        defaults = dict(lr=lr, eps=eps, clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=beta1, weight_decay=weight_decay,
                        scale_parameter=scale_parameter, relative_step=relative_step, warmup_init=warmup_init)
        super().__init__(params, defaults)
        if ctypes.sizeof(_Desc) != _lib.load().fat5_sizeof_adafactor_tensor():
            raise ImportError("fat5_adafactor_tensor layout mismatch between libfat5.so and its binding")

    @staticmethod
    def _schedule(group, step):
        """(beta2t, rho) of step number `step` >= 1: HF's `1 - step ** decay_rate` and the `rel_step_sz` of its `_get_lr` (the
        group's `lr` without `relative_step`), formed in double like HF's Python and cast once by the launch"""
        beta2t = 1.0 - math.pow(step, group["decay_rate"])
        if group["relative_step"]:
            min_step = 1e-6 * step if group["warmup_init"] else 1e-2
            return beta2t, min(min_step, 1.0 / math.sqrt(step))
        return beta2t, float(group["lr"])

    @staticmethod
    def _check(p):
        if p.grad.is_sparse:
            raise RuntimeError("Adafactor does not support sparse gradients.")
        if not p.is_cuda:
            raise RuntimeError("flasht5_amd.Adafactor needs parameters on the HIP device (no CPU fallback)")
        if p.dim() > 2:
            raise RuntimeError("flasht5_amd.Adafactor: parameters with more than two dimensions are not supported")
        if not (p.is_contiguous() and p.grad.is_contiguous()):
            raise RuntimeError("Adafactor: parameters and gradients must be contiguous")

    @staticmethod
    def _init_state(p, state, group):
        """HF's state of one parameter, in fp32 on its device; a state loaded from a checkpoint (of either class) is brought to fp32"""
        f32 = dict(dtype=torch.float32, device=p.device)
        if "step" not in state:
            state["step"] = 0
            state["RMS"] = torch.zeros((), **f32)
            if p.dim() == 2:
                state["exp_avg_sq_row"] = torch.zeros(p.shape[0], **f32)
                state["exp_avg_sq_col"] = torch.zeros(p.shape[1], **f32)
            else:
                state["exp_avg_sq"] = torch.zeros(p.numel(), **f32).view(p.shape)
        if group["beta1"] is not None and "exp_avg" not in state:
            state["exp_avg"] = torch.zeros(p.shape, **f32)
        for key in ("RMS", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "exp_avg"):
            v = state.get(key)
            if key in state and not (torch.is_tensor(v) and v.dtype == torch.float32 and v.device == p.device and v.is_contiguous()):
                state[key] = torch.as_tensor(v, **f32).contiguous()
        state["step"] = int(state["step"])

    @torch.no_grad()
    def init_state(self):
        """allocate the state of every parameter now (what the first step() does lazily) and the arena of a captured step: a step can
        only be captured in a graph once both exist"""
        count = {}
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad and p.is_cuda and p.dim() <= 2:
                    self._init_state(p, self.state[p], group)
                    count[p.device] = count.get(p.device, 0) + 1
        self._reserve_arena({dev: (2 * n + 32 * len(self.param_groups) + 8) * 128 for dev, n in count.items()})

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        todo = []  # (group, parameters with a gradient): everything is checked before anything is launched
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None and p.numel() > 0]
            for p in ps:
                self._check(p)
                if capturing and "step" not in self.state[p]:
                    raise RuntimeError("Adafactor: the optimizer state must exist before a step is captured in a graph "
                                       "(run one eager step first, or call init_state())")
            todo.append((group, ps))
        if capturing:  # (a step recorded into a HIP graph: see graph_advance)
            self._begin_capture()
        for group, ps in todo:
            buckets = {}
            for p in ps:
                state = self.state[p]
                self._init_state(p, state, group)
                if not capturing:
                    state["step"] += 1
                buckets.setdefault((p.device, p.dtype, p.grad.dtype, group["beta1"] is not None), []).append((p, state))
            if capturing and len({self.state[p]["step"] for p in ps}) > 1:  # (the launch reads ONE beta2t / rho per bucket)
                raise RuntimeError("Adafactor: a captured step needs one step count per parameter group")
            for (device, dtype, gdtype, mom), items in buckets.items():
                table = (_Desc * (len(items) + 1))()
                for d, (p, state) in zip(table, items):
                    d.p, d.g, d.rms = p.data_ptr(), p.grad.data_ptr(), state["RMS"].data_ptr()
                    if p.dim() == 2:
                        d.rows, d.cols = p.shape
                        d.vr, d.vc = state["exp_avg_sq_row"].data_ptr(), state["exp_avg_sq_col"].data_ptr()
                    else:
                        d.rows, d.cols = 0, p.numel()
                        d.vr = state["exp_avg_sq"].data_ptr()
                    d.m = state["exp_avg"].data_ptr() if mom else None
                    d.beta2t, d.rho = self._schedule(group, max(state["step"], 1))
                nbytes = lib.fat5_adafactor_workspace_bytes(table, len(items))
                if nbytes == 0:
                    _lib.check(-1, "fat5_adafactor_workspace_bytes")
                ws = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
                scalars = None
                if capturing:
                    # capture runs nothing: the table is uploaded after the capture, in front of the first replay (graph_advance); table
                    # and step scalars live in the arena allocated BEFORE the capture (memory taken from the graph's pool during capture
                    # may alias activations that were freed earlier in the capture)
                    host = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8)
                    raw = self._arena_take(device, host.numel())
                    scalars = self._arena_take(device, 12).view(torch.float32)
                    self._graph_jobs.append((group, [st for _, st in items], scalars, raw, host))
                    self._graph_keep += [ws, [p.grad for p, _ in items]]
                else:
                    raw = self._upload(device, table)
                eps0, eps1 = group["eps"]
                with _lib.on_device(device):
                    _lib.check(lib.fat5_adafactor_step(table, raw.data_ptr(), len(items), ws.data_ptr(), nbytes, float(eps0), float(eps1),
                                                       float(group["clip_threshold"]), float(group["beta1"]) if mom else -1.0,
                                                       float(group["weight_decay"]), int(bool(group["scale_parameter"])),
                                                       _lib.dtype_code(dtype), _lib.dtype_code(gdtype),
                                                       scalars.data_ptr() if scalars is not None else None, _lib.stream_ptr(device)),
                               "fat5_adafactor_step")
                if not capturing:
                    # the kernels write through raw pointers: bump the autograd version of what they changed, so that anything keyed on
                    # (data_ptr, _version) of a parameter -- the FP8 weight cache of generation -- sees the update
                    torch.autograd.graph.increment_version([p for p, _ in items])
        return loss

    @torch.no_grad()
    def graph_advance(self):
        """Before every replay of a graph that holds a captured step(): count the step and write the three step-dependent scalars of
        each bucket -- beta2t, rho (the relative step, or the group's current `lr`), weight_decay -- into its device tensor
        (stream-ordered in front of the replay; the values the eager step passes in the table and as a launch argument)."""
        if not getattr(self, "_graph_jobs", None):
            raise RuntimeError("Adafactor.graph_advance: no captured step")
        for i, (group, states, scalars, raw, host) in enumerate(self._graph_jobs):
            if host is not None:  # first replay: the descriptor table of the bucket
                raw.copy_(host)
                self._graph_jobs[i] = (group, states, scalars, raw, None)
            for st in states:
                st["step"] += 1
            beta2t, rho = self._schedule(group, states[0]["step"])
            # (three fill launches -- the values travel as launch arguments; a copy from a host tensor would wait for the stream)
            for j, val in enumerate((beta2t, rho, float(group["weight_decay"]))):
                scalars[j:j + 1].fill_(val)
