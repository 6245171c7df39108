"""Generic learner over any dueling ``nn.Module`` (CPU path, MLP/IMPALA nets,
and the correctness oracle for the fused MI355X learner).

Reference parity: ``Learner`` (``learner.py:10-80``) -- double-DQN loss
(:29-52), optimizer step + target sync (:54-61), checkpoint load (:18-23).
Fixed: target net starts as a copy of the online net (A30), target sync on
``n % freq == 0`` (A17), centered RMSprop with decay 0.95 (A16), grad-norm
clip, Huber + IS weights (A18), no ``requires_grad_`` on inputs (A20).
Data parallel: gradients are all-reduced across ranks
(``parallel/dist.py``) before the optimizer step.
"""
from __future__ import annotations

import copy
from typing import Any, Dict, Optional

import numpy as np
import torch

from ..config import ApexConfig
from ..models.dueling import build_network
from ..utils.checkpoint import adopt_obs_scale, check_dist_head, check_noisy, load_checkpoint, save_checkpoint
from .losses import c51_loss, ddqn_loss, hl_gauss_loss, munchausen_loss, munchausen_targets, quantile_huber_loss
from .schedules import lr_scheduled, rt_lr, target_ema_on


def make_optimizer(params, rt) -> torch.optim.Optimizer:
    if getattr(rt, "optimizer", "rmsprop") == "adam":
        return torch.optim.Adam(params, lr=rt.lr, betas=(rt.adam_beta1, rt.adam_beta2), eps=rt.adam_eps)
    return torch.optim.RMSprop(params, lr=rt.lr, alpha=rt.rms_decay, eps=rt.rms_eps,
                               centered=rt.centered_rmsprop)


class TorchLearner:
    def __init__(self, cfg: ApexConfig, device: torch.device, comm=None):
        self.cfg = cfg
        self.rt = cfg.Runtime
        self.device = torch.device(device)
        self.comm = comm
        shape = cfg.env_conf.state_shape
        self.Q = build_network(cfg.network, shape, cfg.env_conf.action_dim,
                               obs_scale=self.rt.obs_scale, **cfg.head_kw()).to(self.device)
        if comm is not None and comm.world_size > 1:
            comm.broadcast_module(self.Q)
        self.Q_target = copy.deepcopy(self.Q)
        for p in self.Q_target.parameters():
            p.requires_grad_(False)
        self.optimizer = make_optimizer(self.Q.parameters(), self.rt)
        self.num_q_updates = 0
        ls = cfg.Learner.load_saved_state
        if ls:
            self.load(ls)

    # ---------------------------------------------------------------- io
    def _to(self, x, dtype=None):
        t = torch.as_tensor(x)
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device, non_blocking=True)

    def q_values(self, obs) -> torch.Tensor:
        with torch.no_grad():
            return self.Q(self._to(obs))[2]

    # -------------------------------------------------------------- step
    def compute_loss_and_priorities(self, batch: Dict[str, Any]):
        S_t = self._to(batch["S_t"])
        S_tpn = self._to(batch["S_tpn"])
        P = int(self.rt.augment_shift)
        if P >= 1 and S_t.dim() == 4 and tuple(S_t.shape[2:]) == (84, 84):
            # random-shift augmentation by the fused learner's convention (learner/augment.py: update index =
            # num_q_updates, rows b = S_t, B + b = S_t+n), so both see the same shifted frames
            from .augment import aug_seed, shift_frames, shift_offsets
            B = S_t.shape[0]
            off = shift_offsets(aug_seed(self.rt.seed), self.num_q_updates, 2 * B, P)
            self.last_aug_off = off
            S_t, S_tpn = shift_frames(S_t, off[:B], P), shift_frames(S_tpn, off[B:], P)
        A = self._to(batch["A_t"], torch.long)
        R = self._to(batch["R"], torch.float32)
        G = self._to(batch["Gamma"], torch.float32)
        w = self._to(batch["weights"], torch.float32) if (
            self.rt.use_is_weights and "weights" in batch) else None
        rs = self.cfg.rescale_eps        # Runtime.value_rescale: the rescaled target (learner/rescale.py), or None
        if self.cfg.implicit:
            # IQN: the quantile Huber loss at sampled fractions, three sets per row drawn by the fused learner's
            # convention (learner/iqn.py: update index = num_q_updates), so both see the same fractions
            from .iqn import iqn_seed, learner_taus
            from .losses import iqn_loss
            taus = learner_taus(iqn_seed(self.rt.seed), self.num_q_updates, S_t.shape[0],
                                int(self.rt.num_atoms)).to(self.device)
            self.last_taus = taus
            with torch.no_grad():
                q_next_online = self.Q.quantiles_at(S_tpn, taus[:, 1]).mean(-1)
                th_next_target = self.Q_target.quantiles_at(S_tpn, taus[:, 2])
            return iqn_loss(self.Q.quantiles_at(S_t, taus[:, 0]), taus[:, 0], q_next_online, th_next_target, A, R, G,
                            self.rt.huber_delta, w, rescale_eps=rs)
        if self.cfg.quantile:
            # QR-DQN: quantile Huber loss against the target net's quantiles (learner/losses.py)
            with torch.no_grad():
                q_next_online = self.Q(S_tpn)[2]
                th_next_target = self.Q_target.quantiles(S_tpn)
            return quantile_huber_loss(self.Q.quantiles(S_t), q_next_online, th_next_target, A, R, G,
                                       self.rt.huber_delta, w, rescale_eps=rs)
        if self.cfg.hl_gauss:
            # HL-Gauss: cross-entropy against the Gaussian histogram of the scalar target (learner/losses.py)
            with torch.no_grad():
                q_next_online = self.Q(S_tpn)[2]
                q_next_target = self.Q_target(S_tpn)[2]
            return hl_gauss_loss(self.Q.log_probs(S_t), q_next_online, q_next_target, A, R, G, self.rt.v_min,
                                 self.rt.v_max, self.rt.hl_gauss_sigma_ratio, w, rescale_eps=rs)
        if self.cfg.distributional:
            # C51: cross-entropy against the projected target distribution (learner/losses.py)
            with torch.no_grad():
                q_next_online = self.Q(S_tpn)[2]
                p_next_target = self.Q_target.log_probs(S_tpn).exp()
            return c51_loss(self.Q.log_probs(S_t), q_next_online, p_next_target, A, R, G,
                            self.rt.v_min, self.rt.v_max, w, rescale_eps=rs)
        if self.rt.munchausen:
            # Munchausen-DQN: the target net at S_t and S_t+n, no online argmax (learner/losses.py)
            with torch.no_grad():
                g0 = self.Q_target(S_t)[2]
                g1 = self.Q_target(S_tpn)[2]
                kw = self.cfg.munchausen_kw()
                _, bonus, vsoft = munchausen_targets(g0, g1, A, R, G, **kw)
                self._mdqn = (float(bonus.mean()), float(vsoft.mean()))
            return munchausen_loss(self.Q(S_t)[2], g0, g1, A, R, G, w, loss=self.rt.loss,
                                   kappa=self.rt.huber_delta, **kw)
        with torch.no_grad():
            q_next_online = self.Q(S_tpn)[2]
            q_next_target = self.Q_target(S_tpn)[2]
        q_t = self.Q(S_t)[2]
        return ddqn_loss(q_t, q_next_online, q_next_target, A, R, G, w,
                         loss=self.rt.loss, kappa=self.rt.huber_delta, rescale_eps=rs)

    def update_Q(self, loss: torch.Tensor) -> float:
        self.optimizer.zero_grad(set_to_none=False)
        loss.backward()
        if self.comm is not None and self.comm.world_size > 1:
            self.comm.allreduce_grads([p.grad for p in self.Q.parameters()])
        gnorm = 0.0
        if self.rt.grad_clip and self.rt.grad_clip > 0:
            gnorm = float(torch.nn.utils.clip_grad_norm_(self.Q.parameters(), self.rt.grad_clip))
        if lr_scheduled(self.rt):
            for gr in self.optimizer.param_groups:
                gr["lr"] = rt_lr(self.rt, self.num_q_updates)
        self.optimizer.step()
        self.num_q_updates += 1
        if target_ema_on(self.rt):
            self.ema_target()
        elif self.num_q_updates % self.cfg.Learner.q_target_sync_freq == 0:
            self.sync_target()
        I = int(self.rt.reset_interval)
        if I and self.num_q_updates % I == 0:
            self.reset_now(self.num_q_updates // I)
        return gnorm

    def reset_now(self, r: int) -> None:
        """Shrink-and-perturb reset ``r`` (Runtime.reset_interval, learner/reset.py) by the fused learner's
        convention on this module's parameters in ``named_parameters()`` order (flat index = running offset,
        fan-in from the shape, ``module_reset_table``): both nets mixed with the same fresh values, the optimizer
        state dropped (zero moments, Adam's step count restarts)."""
        from .reset import apply_reset, module_reset_table, reset_seed
        table = module_reset_table(self.Q, self.cfg)
        tgt = dict(self.Q_target.named_parameters())
        pairs = [(p, tgt[k]) for k, p in self.Q.named_parameters()]
        flat = [np.concatenate([x.detach().cpu().numpy().ravel() for x in col]).astype(np.float32)
                for col in zip(*pairs)]
        zero = np.zeros_like(flat[0])
        apply_reset(flat[0], flat[1], zero, zero.copy(), reset_seed(self.rt.seed), int(r), table)
        with torch.no_grad():
            for row, (p, t) in zip(table, pairs):
                for x, a in ((p, flat[0]), (t, flat[1])):
                    x.copy_(torch.from_numpy(a[row.start:row.end]).reshape(x.shape))
        self.optimizer.state.clear()

    def ema_target(self) -> None:
        """The soft target (Runtime.target_ema_rate): every parameter of the target module averaged with the
        online one just written -- learner/schedules.py ``target_ema`` in tensor operations (two fp32
        products and a sum, no addcmul / lerp).  It replaces the hard sync."""
        r = torch.tensor(float(self.rt.target_ema_rate), dtype=torch.float32, device=self.device)
        a = torch.ones_like(r) - r
        with torch.no_grad():
            for t, p in zip(self.Q_target.parameters(), self.Q.parameters()):
                ta = t * a
                pr = p.detach() * r
                torch.add(ta, pr, out=t)

    def sync_target(self) -> None:
        self.Q_target.load_state_dict(self.Q.state_dict())

    def set_update_noise(self) -> None:
        """Noisy layers: the draws of update ``num_q_updates`` -- the online net's (s = 0, both
        its S_t and S_t+n rows) and the target net's (s = 1); the fused learner's convention
        (learner/noisy.py), so both see the same noise."""
        if self.rt.noisy:
            from .noisy import set_module_noise
            set_module_noise(self.Q, self.rt.seed, self.num_q_updates, 0)
            set_module_noise(self.Q_target, self.rt.seed, self.num_q_updates, 1)

    def step(self, batch: Dict[str, Any]) -> Dict[str, Any]:
        self.set_update_noise()
        loss, td = self.compute_loss_and_priorities(batch)
        gnorm = self.update_Q(loss)
        out = {"loss": float(loss.detach()), "td_abs": td.cpu().numpy(), "grad_norm": gnorm}
        out.update(self.last_metrics())
        return out

    def last_metrics(self) -> Dict[str, float]:
        """Munchausen target: the last update's mean bonus and mean soft value; Runtime.reset_interval: the
        resets so far (else empty)."""
        m = {}
        if int(self.rt.reset_interval) > 0:
            m["resets"] = self.num_q_updates // int(self.rt.reset_interval)
        if self.rt.munchausen and getattr(self, "_mdqn", None) is not None:
            m.update(munchausen_bonus_mean=self._mdqn[0], soft_value_mean=self._mdqn[1])
        return m

    # --------------------------------------------------------- params
    def state_dict_for_actors(self) -> Dict[str, torch.Tensor]:
        return {k: v.detach() for k, v in self.Q.state_dict().items()}

    def save(self, path: str, extras: bool = True) -> None:
        ex: Dict[str, Any] = {}
        if extras:
            ex = dict(Q_target_state=self.Q_target.state_dict(),
                      optimizer_state=self.optimizer.state_dict(), optimizer_kind=str(self.rt.optimizer),
                      num_q_updates=self.num_q_updates,
                      config=self.cfg.to_dict())
        save_checkpoint(path, self.Q.state_dict(), **ex)

    def load(self, path: str) -> bool:
        ck = load_checkpoint(path)
        if ck is None:
            return False
        check_dist_head(ck, self.rt)
        check_noisy(ck, self.rt)
        if adopt_obs_scale(ck, self.rt):
            for net in (self.Q, self.Q_target):
                if hasattr(net, "pre"):
                    net.pre.scale = self.rt.obs_scale
        self.Q.load_state_dict(ck["Q_state"])
        if "Q_target_state" in ck:
            self.Q_target.load_state_dict(ck["Q_target_state"])
        else:
            self.sync_target()
        if "optimizer_state" in ck:
            saved = str(ck.get("optimizer_kind", "rmsprop"))     # (untagged / older: rmsprop)
            if saved == self.rt.optimizer:
                self.optimizer.load_state_dict(ck["optimizer_state"])
            else:
                print(f"WARNING: checkpoint optimizer state is {saved} state, this learner runs "
                      f"{self.rt.optimizer}; optimizer state not restored (starts fresh)")
        self.num_q_updates = int(ck.get("num_q_updates", 0))
        return True
