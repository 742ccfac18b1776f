"""Dynamic loss scale for the fused training step: torch.amp.GradScaler's rule, kept and applied ON THE DEVICE.

The step is a static list of launches that can replay as one hipGraph with no host read, so the host cannot look at a found-inf flag and decide:
the state -- scale, growth tracker, found-inf word, the count `t` of Adam updates actually applied, the count of skipped steps -- lives in 64 bytes of
device memory (`mtbc_loss_scale_state`), and three small launches per step work on it (include/mtbc.h):

    begin : *gscale = shard_weight * scale (the word the loss-gradient kernels multiply by); Adam's three scalars for step t + 1, in double
    check : one pass over the flat gradient buffer, found_inf = 1 on any inf / NaN (after the all-reduce under data parallel: every rank sees it)
    apply : the fused optimizer launch (Adam, SGD or AdamW; mtbc_loss_scale_optim), every thread returning at once when found_inf is set; then the update rule on the state

State dicts use torch.amp.GradScaler's keys, so the two interchange.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib as L

_LR, _SHARD = 5, 6        # float word index of mtbc_loss_scale_state.lr / .shard_weight


def betas_of(optimizer):
    """The betas `begin` evaluates the bias corrections with: the optimizer's, where it has any (FusedSGD: torch.optim.Adam's defaults, not read)."""
    return tuple(optimizer.param_groups[0].get("betas", (0.9, 0.999)))


class DynamicLossScale:
    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000):
        if not (init_scale > 0.0 and float(init_scale) < float("inf")):
            raise ValueError("init_scale must be positive and finite")
        if growth_factor <= 1.0:
            raise ValueError("The growth factor must be > 1.0.")          # torch.amp.GradScaler's own conditions
        if not (0.0 < backoff_factor < 1.0):
            raise ValueError("The backoff factor must be in (0, 1).")
        if int(growth_interval) < 1:
            raise ValueError("growth_interval must be >= 1")
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._host = L.LossScaleState()              # what the device state starts from (and the only copy while there is no device buffer yet)
        self._host.scale, self._host.shard_weight = float(init_scale), 1.0
        self._state: Optional[torch.Tensor] = None   # 16 int32 words on the device = mtbc_loss_scale_state
        self._f: Optional[torch.Tensor] = None       # the same memory as float32

    # ---- device state ---------------------------------------------------------------------------------------------------------
    def ensure(self, device) -> torch.Tensor:
        """The device copy of the state (created from the host copy at first use, moved along when the model changes device)."""
        device = torch.device(device)
        if self._state is None or self._state.device != device:
            if self._state is not None:
                self._pull()
            words = torch.frombuffer(bytearray(bytes(self._host)), dtype=torch.int32).clone()
            self._state = words.to(device)
            self._f = self._state.view(torch.float32)
        return self._state

    def _pull(self) -> "L.LossScaleState":
        if self._state is not None:
            self._host = L.LossScaleState.from_buffer_copy(self._state.cpu().numpy().tobytes())
        return self._host

    def _push(self) -> None:
        if self._state is not None:
            self._state.copy_(torch.frombuffer(bytearray(bytes(self._host)), dtype=torch.int32))

    def stats(self) -> Dict[str, float]:
        """One device -> host read (a synchronisation: for logs and tests, never called by the step)."""
        h = self._pull()
        return {"scale": float(h.scale), "growth_tracker": int(h.growth_tracker), "skipped": int(h.skipped), "t": int(h.t)}

    def set_t(self, t: int) -> None:
        """The number of Adam updates already applied (a resumed optimizer state carries it as `step`)."""
        self._pull().t = int(t)
        self._push()

    def attach(self, optimizer) -> None:
        """The optimizer whose step count this scale owns from now on: `t` starts from the optimizer's own count (a resumed run), the optimizer's
        `state_dict()` reads it back from the device."""
        if getattr(optimizer, "_loss_scaler", None) is not self:
            optimizer._loss_scaler = self
            if int(self._host.t) == 0 and int(getattr(optimizer, "step_count", 0)) > 0 and self._state is None:
                self._host.t = int(optimizer.step_count)

    def graph_key(self):
        return (self._state.data_ptr(), self.growth_factor, self.backoff_factor, self.growth_interval)

    # ---- the per-step launches (all stream-ordered; begin / check / apply are capturable, the two fills are not meant to be) ---------------------------
    def set_lr(self, lr: float) -> None:
        self._f[_LR:_LR + 1].fill_(float(lr))

    def set_shard_weight(self, w: float) -> None:
        self._f[_SHARD:_SHARD + 1].fill_(float(w))

    def args(self, world: int = 1, betas=(0.9, 0.999), gscale_out: Optional[torch.Tensor] = None, g: Optional[torch.Tensor] = None) -> "L.LossScaleArgs":
        a = L.LossScaleArgs()
        a.state = self._state.data_ptr()
        a.gscale_out = gscale_out.data_ptr() if gscale_out is not None else None
        if g is not None:
            a.g, a.n = g.data_ptr(), g.numel()
        a.growth_factor, a.backoff_factor, a.growth_interval = self.growth_factor, self.backoff_factor, self.growth_interval
        a.inv_world, (a.beta1, a.beta2) = 1.0 / world, betas
        return a

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def begin(self, gscale_out: torch.Tensor, world: int, betas) -> None:
        L.check(L.load().mtbc_loss_scale_begin(C.byref(self.args(world, betas, gscale_out=gscale_out)), self._stream()), "loss scale begin")

    def check(self, flat_g: torch.Tensor) -> None:
        L.check(L.load().mtbc_loss_scale_check(C.byref(self.args(g=flat_g)), self._stream()), "loss scale check")

    def apply(self, optimizer, world: int) -> None:
        """The optimizer's fused launch under the found-inf word, then the update of the state (lr, step and grad_scale of the arguments are not read)."""
        optimizer._ensure_state()
        L.check(L.load().mtbc_loss_scale_optim(C.byref(self.args(world, betas_of(optimizer))), C.byref(optimizer._args()), self._stream()), "loss scale optim")

    # ---- torch.amp.GradScaler's state dict ---------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        h = self._pull()
        return {"scale": float(h.scale), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(h.growth_tracker)}

    def load_state_dict(self, sd: dict) -> None:
        if len(sd) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        h = self._pull()
        h.scale, h.growth_tracker = float(sd["scale"]), int(sd["_growth_tracker"])
        self.growth_factor, self.backoff_factor, self.growth_interval = float(sd["growth_factor"]), float(sd["backoff_factor"]), int(sd["growth_interval"])
        self._push()
