"""Fused Adam, SGD (Nesterov) and AdamW over the model's flat parameter buffer (one launch for all ~15 M parameters).

Replaces torch.optim.Adam(model.parameters(), lr, eps=1e-4) of src/utils/experiment_init.py:186-187 and its
`.step()` at training_multitask.py:103.  Subclasses torch.optim.Optimizer so ReduceLROnPlateau / CosineAnnealingLR
(experiment_init.py:275-278) and `.param_groups[0]['lr']`, `.zero_grad(set_to_none=True)`, `.state_dict()` work.

FusedSGD / FusedAdamW are the other two names of `optimizer.opt` (experiment_init.py:188-195).  All three are one launch of the same kernel
(mtbc_optim_step; Adam is its AdamW rule with weight_decay 0) behind one base class, so the fused training step drives them alike; their state
dicts are torch.optim.Adam's / torch.optim.SGD's / torch.optim.AdamW's.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L


def _gather_grads(m) -> None:
    """Drop-in path: autograd may have stored p.grad outside the flat gradient buffer -> gather."""
    params = dict(m.named_parameters())
    for name in m._order:
        p, slot = params[name], m._grad_view(name)
        if p.grad is None:
            slot.zero_()
        elif p.grad.data_ptr() != slot.data_ptr():
            slot.copy_(p.grad)


class _FusedFlat(torch.optim.Optimizer):
    """What FusedAdam, FusedSGD and FusedAdamW share: the flat state buffers, the mtbc_optim_args launch in its three forms (launch arguments, 16 bytes of device
    scalars for a replayed step, a dynamic loss scale's state) and the per-parameter state dict of the matching torch optimizer."""
    KIND = None
    STATE = ()                           # (attribute of the flat buffer = key of torch's per-parameter state), in mtbc_optim_args order: m, v
    HAS_STEP = False                     # torch's per-parameter state carries 'step'

    def __init__(self, model, defaults):
        self.model = model
        super().__init__(list(model.parameters()), defaults)
        self.step_count = 0
        for k in self.STATE:
            setattr(self, k, None)
        self.grad_scale = 1.0            # set to 1/world_size by the data-parallel trainer
        self._loss_scaler = None         # a loss_scale.DynamicLossScale (set by the trainer): the count of applied updates then lives on the device
        self._dyn = None

    def _buffers(self):
        return [getattr(self, k) for k in self.STATE]

    def _ensure_state(self) -> None:
        m = self.model
        m.ensure_flat()
        b = self._buffers()[0]
        if b is None or b.device != m.flat_p.device or b.numel() != m.flat_numel:
            for k in self.STATE:
                setattr(self, k, torch.zeros_like(m.flat_p))

    def _hyper(self, a: "L.OptimArgs", g: dict) -> None:
        raise NotImplementedError

    def _args(self) -> "L.OptimArgs":
        m, g = self.model, self.param_groups[0]
        a = L.OptimArgs()
        # the live prefix of the flat buffers: parameters the forward never reads (nets.nnUNetClassifier's decoder4 .. 1) lie behind it and are not
        # touched -- torch's optimizers skip a `.grad` of None, AdamW's decay included; every other model's prefix is the whole buffer
        a.kind, a.n, a.p, a.g = self.KIND, getattr(m, "live_numel", m.flat_numel), m.flat_p.data_ptr(), m.flat_g.data_ptr()
        bufs = self._buffers()
        a.m = bufs[0].data_ptr()
        a.v = bufs[1].data_ptr() if len(bufs) > 1 else None
        a.lr, a.grad_scale, a.step, a.zero_grad = float(g["lr"]), float(self.grad_scale), max(1, self.step_count), 0
        self._hyper(a, g)
        return a

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @torch.no_grad()
    def step(self, closure=None, grads_in_flat: bool = False):
        loss = closure() if closure is not None else None
        self._ensure_state()
        if not grads_in_flat:
            _gather_grads(self.model)
        self.step_count += 1
        L.check(L.load().mtbc_optim_step(C.byref(self._args()), self._stream()), type(self).__name__)
        return loss

    # ---- the step as two halves, for a training step replayed as a hipGraph (trainer.FusedTrainStep(graph=True)): the four scalars that change from
    #      step to step (grad_scale, the step size, 1 / sqrt(1 - b2^t), AdamW's decay factor) travel through 16 bytes of device memory instead of the
    #      launch arguments
    @torch.no_grad()
    def advance_dynamic(self) -> None:
        """Count the step and put its scalars where `launch_dynamic`'s kernel reads them -- four fills in stream order (values in the launch arguments of
        torch's fill kernel: no host buffer that a later step could overwrite while a copy is in flight).  NOT captured."""
        self._ensure_state()
        if self._dyn is None or self._dyn.device != self.model.flat_p.device:
            self._dyn = torch.zeros(4, device=self.model.flat_p.device)
        self.step_count += 1
        out = (C.c_float * 4)()
        L.check(L.load().mtbc_optim_dynamic(C.byref(self._args()), C.byref(out)), "optimizer scalars")
        for i in range(4):
            self._dyn[i:i + 1].fill_(float(out[i]))           # a float32 value passed as a double: exact

    @torch.no_grad()
    def launch_dynamic(self) -> None:
        """The launch itself, reading the scalars `advance_dynamic` left: the same kernel, the same bits as `step`.  Capturable."""
        a = self._args()
        a.dynamic = self._dyn.data_ptr()
        L.check(L.load().mtbc_optim_step(C.byref(a), self._stream()), type(self).__name__)

    def _hyper_key(self):
        raise NotImplementedError

    def graph_key(self, dynamic: bool = True):
        """What a captured launch_dynamic holds by address or by value (dynamic=False: without the 16 bytes of scalars)."""
        return (self.model.flat_p.data_ptr(), self.model.flat_g.data_ptr(), *(b.data_ptr() for b in self._buffers()),
                self._dyn.data_ptr() if dynamic else None, *self._hyper_key())

    def applied_steps(self) -> int:
        """Updates applied so far: the host's count, or the device's under a dynamic loss scale (one read-back; skipped steps do not count)."""
        if self._loss_scaler is not None:
            self.step_count = int(self._loss_scaler.stats()["t"])
        return self.step_count

    # ---- checkpoint interchange (training_multitask.py:243-249 saves `optimizer.state_dict()`): torch's own layout, per-parameter state keyed by
    #      parameter index, so a reference checkpoint resumes here and a checkpoint written here resumes under the matching torch optimizer
    def state_dict(self):
        sd = super().state_dict()
        if self._buffers()[0] is not None and self.applied_steps() > 0:
            m = self.model
            state = {}
            for i, name in enumerate(n for n, _ in m.named_parameters()):
                if name in getattr(m, "untrained", ()):        # never stepped: torch keeps no state for it either
                    continue
                s = m.slots[name]
                state[i] = {"step": torch.tensor(float(self.step_count))} if self.HAS_STEP else {}
                for k in self.STATE:
                    state[i][k] = getattr(self, k)[s.offset:s.offset + s.numel].view(s.shape).detach().clone()
            sd["state"] = state
        return sd

    def load_state_dict(self, sd):
        state = sd.get("state", {}) or {}
        super().load_state_dict({"state": {}, "param_groups": sd["param_groups"]})
        m = self.model
        if not state:
            return
        self._ensure_state()
        steps = set()
        for i, name in enumerate(n for n, _ in m.named_parameters()):
            st = state.get(i, state.get(str(i)))
            if st is None or name in getattr(m, "untrained", ()):
                continue
            s = m.slots[name]
            for k in self.STATE:
                if st.get(k) is not None:                      # torch.optim.SGD keeps None until a parameter's first step
                    getattr(self, k)[s.offset:s.offset + s.numel].copy_(st[k].reshape(-1))
            if self.HAS_STEP:
                steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): not a state this optimizer can hold")
        if self.HAS_STEP:
            self.step_count = steps.pop() if steps else 0
            if self._loss_scaler is not None:
                self._loss_scaler.set_t(self.step_count)
        elif self.applied_steps() < 1:
            self.step_count = 1                                # torch.optim.SGD's state carries no count: at least one update was applied
            if self._loss_scaler is not None:                  # (a device count that is already there stays)
                self._loss_scaler.set_t(1)


class FusedSGD(_FusedFlat):
    """torch.optim.SGD(lr, momentum=0.9, nesterov=True) of experiment_init.py:188-189 (dampening 0, weight_decay 0) as one launch."""
    KIND = L.OPT_SGD
    STATE = ("momentum_buffer",)

    def __init__(self, model, lr: float = 1e-3, momentum: float = 0.9, nesterov: bool = True):
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")       # torch.optim.SGD's own condition
        # the full hyper-parameter set of the installed torch.optim.SGD, so that `state_dict()['param_groups']` loads into one
        ref = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr, momentum=momentum, nesterov=nesterov)
        super().__init__(model, dict(ref.defaults))

    def _hyper(self, a, g):
        if g.get("weight_decay", 0) or g.get("dampening", 0) or g.get("maximize", False):
            raise NotImplementedError("FusedSGD is the reference's SGD: weight_decay 0, dampening 0, maximize False")
        a.momentum, a.nesterov = float(g["momentum"]), int(bool(g["nesterov"]))
        a.beta1, a.beta2 = 0.9, 0.999                           # not read by the kernel

    def _hyper_key(self):
        g = self.param_groups[0]
        return (float(g["momentum"]), bool(g["nesterov"]))


class FusedAdam(_FusedFlat):
    """torch.optim.Adam(lr, eps=1e-4) of experiment_init.py:186-187 as one launch: the AdamW rule with weight_decay 0, whose decay factor
    (float)(1 - lr * 0) = 1 leaves every parameter word as it is."""
    KIND = L.OPT_ADAMW
    STATE = ("exp_avg", "exp_avg_sq")
    HAS_STEP = True

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        # the full hyper-parameter set of the installed torch.optim.Adam, so that `state_dict()['param_groups']` loads into one
        ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps)
        super().__init__(model, dict(ref.defaults))

    def _hyper(self, a, g):
        (a.beta1, a.beta2), a.eps, a.weight_decay = g["betas"], float(g["eps"]), 0.0      # the group's weight_decay is not read: this is Adam as the reference runs it

    def _hyper_key(self):
        g = self.param_groups[0]
        return (tuple(g["betas"]), float(g["eps"]))

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        legacy = sd.get("fused")                       # round-1 private format: the step count and the two flat buffers
        if legacy is not None and not sd.get("state"):
            self.step_count = int(legacy["step"])
            if self._loss_scaler is not None:
                self._loss_scaler.set_t(self.step_count)
            if legacy["exp_avg"] is not None:
                self._ensure_state()
                self.exp_avg.copy_(legacy["exp_avg"])
                self.exp_avg_sq.copy_(legacy["exp_avg_sq"])


class FusedAdamW(_FusedFlat):
    """torch.optim.AdamW(lr) of experiment_init.py:190-191 (betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2) as one launch."""
    KIND = L.OPT_ADAMW
    STATE = ("exp_avg", "exp_avg_sq")
    HAS_STEP = True

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2):
        ref = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(model, dict(ref.defaults))

    def _hyper(self, a, g):
        if g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError("FusedAdamW: amsgrad False, maximize False")
        (a.beta1, a.beta2), a.eps, a.weight_decay = g["betas"], float(g["eps"]), float(g["weight_decay"])

    def _hyper_key(self):
        g = self.param_groups[0]
        return (tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"]))


FUSED_OPTIMIZERS = (FusedAdam, FusedSGD, FusedAdamW)
