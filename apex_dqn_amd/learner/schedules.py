"""Step-indexed schedules of the learner update: learning rate, IS exponent, Adam's bias
corrections -- the host mirror of csrc/rmsprop_common.h (``sched_lr``, ``sched_beta``,
``pow_u64``).

``u`` is the number of updates completed before the current one.  The kernels evaluate
the schedules in fp64 from the integer index and round once to fp32; the functions here
do the same operations in the same order in numpy float64, so device and host agree bit
for bit.  Inside a replayed graph the index comes from device memory: the replay's draw
counter (bumped once per update by the priority write-back, ahead of the optimizer
launch) minus a base word the learner sets at construction / load (:class:`OptSpec`).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

OPTIMIZERS = ("rmsprop", "adam")


def lr_at(u: int, lr: float, warmup: int = 0, decay: int = 0, lr_end: Optional[float] = None) -> np.float32:
    """lr(u): linear warm-up over ``warmup`` updates, then a linear ramp to ``lr_end`` over
    ``decay`` updates (0: constant)."""
    u, warmup, decay = int(u), int(warmup), int(decay)
    lr0 = np.float64(lr)
    if u < warmup:
        v = lr0 * np.float64(u + 1) / np.float64(warmup)
    elif decay > 0:
        end = np.float64(lr if lr_end is None else lr_end)
        v = lr0 + (end - lr0) * min(np.float64(1.0), np.float64(u - warmup) / np.float64(decay))
    else:
        v = lr0
    return np.float32(v)


def beta_at(u: int, beta0: float, beta_end: Optional[float] = None, steps: int = 0) -> np.float32:
    """IS exponent of the batch update ``u`` consumes (no schedule: ``beta0``)."""
    b0 = np.float64(beta0)
    if beta_end is None:
        return np.float32(b0)
    f = min(np.float64(1.0), np.float64(int(u)) / np.float64(int(steps))) if int(steps) > 0 else np.float64(1.0)
    return np.float32(b0 + (np.float64(beta_end) - b0) * f)


def pow_int(b: float, t: int) -> np.float64:
    """``b ** t`` in fp64 by squaring, in the kernels' multiplication order."""
    r, b, t = np.float64(1.0), np.float64(b), int(t)
    with np.errstate(under="ignore"):
        while t:
            if t & 1:
                r = r * b
            b = b * b
            t >>= 1
    return r


def adam_corrections(u: int, beta1: float, beta2: float, t0: int = 0):
    """(c1, c2) = fp32(1 - beta^t), t = u + 1 - t0 (``t0``: the updates completed at the last shrink-and-perturb
    reset, learner/reset.py -- the moments restart at zero there, so the step count does)."""
    t = max(int(u) + 1 - int(t0), 1)
    return np.float32(np.float64(1.0) - pow_int(beta1, t)), np.float32(np.float64(1.0) - pow_int(beta2, t))


def target_ema(t, p, rho: float) -> np.ndarray:
    """The soft (Polyak) target after an update, ``Runtime.target_ema_rate`` = ``rho``: on fp32 arrays
    ``t`` (the target) and ``p`` (the weights the optimizer has just written),
    ``t' = fl(fl(a t) + fl(r p))`` with ``r = fp32(rho)`` and ``a = fl(1 - r)`` formed once -- two
    products and a sum, each rounded to fp32 (csrc/rmsprop_common.h EMA: no contraction).  ``rho = 1``
    gives ``p`` exactly.  Returns a new fp32 array."""
    t, p = np.asarray(t), np.asarray(p)
    if t.dtype != np.float32 or p.dtype != np.float32:
        raise TypeError("target_ema mirrors fp32 arithmetic: pass float32 arrays")
    r = np.float32(rho)
    a = np.float32(np.float32(1.0) - r)
    ta = (a * t).astype(np.float32)
    pr = (r * p).astype(np.float32)
    return (ta + pr).astype(np.float32)


def target_ema_on(rt) -> bool:
    return float(getattr(rt, "target_ema_rate", 0.0)) > 0.0


def rt_lr(rt, u: int) -> float:
    """lr(u) of a ``Runtime`` section."""
    return float(lr_at(u, rt.lr, rt.lr_warmup_steps, rt.lr_decay_steps, rt.lr_end))


def rt_beta(rt, beta0: float, u: int) -> float:
    """beta(u) of a ``Runtime`` section (``beta0``: Replay_Memory.importance_sampling_exponent)."""
    return float(beta_at(u, beta0, rt.is_beta_end, rt.is_beta_anneal_steps))


def lr_scheduled(rt) -> bool:
    return int(rt.lr_warmup_steps) > 0 or int(rt.lr_decay_steps) > 0


def beta_scheduled(rt) -> bool:
    return rt.is_beta_end is not None


@dataclass
class OptSpec:
    """What an optimizer launch needs beyond the RMSprop scalars: the rule, the lr
    schedule, Adam's constants and the device words of the update index (``ctr`` - ``base``
    - 1 = u inside the update's optimizer launch).  ``ops.optimizer(..., opt=None)`` is the
    RMSprop update with a constant learning rate."""
    kind: str
    ctr: torch.Tensor           # int64 [1]: the replay's draw counter
    base: torch.Tensor          # int64 [1]: the counter at update 0
    lr: float
    warmup: int = 0
    decay: int = 0
    lr_end: Optional[float] = None
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1.5e-4
    t0: Optional[torch.Tensor] = None   # int64 [1]: the updates completed at the last reset (None: 0), Adam only

    @property
    def adam(self) -> bool:
        return self.kind == "adam"

    def index(self) -> torch.Tensor:
        """u as an int64 tensor (no host sync), read where the optimizer launch reads it."""
        return (self.ctr.reshape(-1)[0] - self.base.reshape(-1)[0] - 1).clamp_min(0)

    def lr_tensor(self) -> torch.Tensor:
        """lr(u) as an fp32 tensor: :func:`lr_at` in tensor operations."""
        u = self.index().double()
        lr0 = torch.full_like(u, self.lr)
        out = lr0
        if self.decay > 0:
            end = self.lr if self.lr_end is None else self.lr_end
            out = lr0 + (end - self.lr) * torch.clamp((u - self.warmup) / float(self.decay), max=1.0)
        if self.warmup > 0:
            out = torch.where(u < self.warmup, lr0 * (u + 1) / float(self.warmup), out)
        return out.float()

    def corrections(self):
        """Adam's (c1, c2) as fp32 tensors (torch's fp64 pow: within an ulp of the kernels'
        product chain before the rounding to fp32)."""
        t = self.index().double() + 1
        if self.t0 is not None:
            t = (t - self.t0.reshape(-1)[0].double()).clamp_min(1)
        one = torch.ones_like(t)
        return ((one - torch.full_like(t, self.beta1) ** t).float(),
                (one - torch.full_like(t, self.beta2) ** t).float())


def opt_spec(rt, replay, base: torch.Tensor, t0: Optional[torch.Tensor] = None) -> Optional[OptSpec]:
    """The :class:`OptSpec` of a ``Runtime`` section, or None for the default (RMSprop,
    constant lr): the step then issues exactly the launches of before.  ``t0``: the reset word, which only
    Adam reads."""
    if rt.optimizer == "rmsprop" and not lr_scheduled(rt):
        return None
    t0 = t0 if rt.optimizer == "adam" else None
    return OptSpec(kind=rt.optimizer, ctr=replay.ctr, base=base, lr=float(rt.lr), warmup=int(rt.lr_warmup_steps),
                   decay=int(rt.lr_decay_steps), lr_end=None if rt.lr_end is None else float(rt.lr_end),
                   beta1=float(rt.adam_beta1), beta2=float(rt.adam_beta2), adam_eps=float(rt.adam_eps), t0=t0)


class StepIndexMixin:
    """The device-resident update index of a learner with ``self.rt``, ``self.replay`` and
    ``self.num_q_updates``: ``replay.ctr - upd_base`` equals ``num_q_updates`` at every
    update boundary (the priority write-back bumps the counter once per update; snapshots
    and restores carry the counter).  :meth:`_init_step_index` goes after ``num_q_updates``
    is set, :meth:`_sync_update_index` after every host-side change of either number
    (``load``).  With ``Runtime.reset_interval`` = I > 0 it also owns ``upd_t0``, the updates completed at the last
    reset, (num_q_updates // I) I -- derived, so a checkpoint needs no key for it."""

    upd_t0 = None

    def _init_step_index(self) -> None:
        rt, rp = self.rt, self.replay
        self.upd_base = torch.zeros(1, dtype=torch.int64, device=rp.ctr.device)
        if int(getattr(rt, "reset_interval", 0)) > 0:
            self.upd_t0 = torch.zeros(1, dtype=torch.int64, device=rp.ctr.device)
        self._opt = opt_spec(rt, rp, self.upd_base, self.upd_t0)
        if beta_scheduled(rt):
            rp.set_beta_schedule(self.upd_base, rt.is_beta_end, rt.is_beta_anneal_steps)
        self._sync_update_index()

    def _sync_update_index(self) -> None:
        self.upd_base.copy_(self.replay.ctr - int(self.num_q_updates))
        if self.upd_t0 is not None:
            I = int(self.rt.reset_interval)
            self.upd_t0.fill_(int(self.num_q_updates) // I * I)

    def update_index(self) -> int:
        """The device's update index (a host read-back: tests, diagnostics)."""
        return int((self.replay.ctr - self.upd_base).item())

    def _opt_kw(self) -> dict:
        """``opt=`` of ``ops.optimizer`` (empty for the default: the launches of before)."""
        return {"opt": self._opt} if self._opt is not None else {}

    def schedule_metrics(self) -> dict:
        """lr and IS exponent of the last completed update, from the host mirror."""
        u = max(int(self.num_q_updates) - 1, 0)
        return {"lr": rt_lr(self.rt, u), "is_beta": rt_beta(self.rt, float(self.replay.beta), u)}

    def _opt_kind(self) -> str:
        return str(self.rt.optimizer)
