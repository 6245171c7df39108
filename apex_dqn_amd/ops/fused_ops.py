"""Backends for the fused NatureCNN learner step.

``TorchBackend`` -- every op in PyTorch (CPU path, and the oracle);
``HipBackend``   -- the MI355X path: hand-written gfx950 kernels from
                    ``libapex_kernels.so`` for every op that has one.

Both write into preallocated output buffers so a whole learner step can be
captured in one HIP graph.

fp32-accurate ("split") mode: every activation, gradient and bf16 weight copy
comes as a hi plane (the usual tensor) plus a ``*_lo`` plane with
``value = hi + lo`` (csrc/mfma_common.h ``split_pk_bf16``).  The HIP kernels run
three bf16 MFMAs per fragment pair (hi.hi + lo.hi + hi.lo, fp32 accumulation); the
torch backend emulates the mode by joining the planes into fp32, computing in
fp32 and splitting the outputs again, so the learner's split plumbing runs (and is
tested) on the CPU.  Without ``*_lo`` arguments every op is the plain bf16 / fp32
op of before.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from . import conv as C
from . import reference as R
from ..learner.rescale import rescale_target
from .switches import SW


def join(hi: torch.Tensor, lo: Optional[torch.Tensor], dtype=torch.float32) -> torch.Tensor:
    """hi (+ lo) as fp32, or as ``dtype`` (the heads' fp64 reference)."""
    return hi.to(dtype) if lo is None else hi.to(dtype) + lo.to(dtype)


def _head_dtype(t: torch.Tensor):
    """fp64 when ``t`` (a head weight, or the Munchausen head's activations) is fp64 -- the tests' reference --
    else fp32."""
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def split_into(v: torch.Tensor, hi: torch.Tensor, lo: Optional[torch.Tensor]) -> None:
    """Write fp32 ``v`` as hi = round(v), lo = round(v - hi) (or just hi when lo is None)."""
    hi.copy_(v.reshape(hi.shape))
    if lo is not None:
        lo.copy_((v.reshape(hi.shape).float() - hi.float()))


def _sample5(sample):
    """``(replay, B, out, nxt2, obs2)`` of an optimizer call's ``sample`` (``obs2`` optional)."""
    return tuple(sample) + (None,) * (5 - len(sample))


class TorchBackend:
    name = "torch"

    def __init__(self, dtype=torch.float32):
        self.dtype = dtype

    # ------------------------------------------------------------- forward
    def prepare(self, Pb) -> None:
        """Per-step weight preparation (nothing on either backend: the dgrad GEMMs read
        the natural weight tensors)."""

    def conv1_fwd(self, frames, w, b, scale, out, out_lo=None):
        dt = torch.float32 if out_lo is not None else self.dtype
        split_into(R.conv1_fwd(frames, w, b, scale, dt), out, out_lo)

    def conv1_fwd_ring(self, ring, slots, frames_buf, w, b, scale, out, w2=None, b2=None, rows_first=0, w32=None,
                       w2_32=None, out_lo=None, c2f=None):
        """conv1 on frame stacks addressed by replay-ring slots (N, C); rows >=
        ``rows_first`` use the second weight set (w2, b2) when given.  Split mode reads
        the fp32 master weights ``w32`` / ``w2_32``.  ``c2f``: conv2 weights the HIP
        backend pre-packs inside this launch (ignored here)."""
        from ..replay.gpu_replay import from_s2d
        frames = frames_buf[:slots.shape[0]]
        n, c = slots.shape
        frames.copy_(from_s2d(ring[slots.long()].reshape(n * c, 84, 84)).reshape(n, c, 84, 84))
        wa, wb = (w32, w2_32) if out_lo is not None else (w, w2)
        if w2 is None:
            self.conv1_fwd(frames, wa, b, scale, out, out_lo)
        else:
            r = rows_first
            self.conv1_fwd(frames[:r], wa, b, scale, out[:r], None if out_lo is None else out_lo[:r])
            self.conv1_fwd(frames[r:], wb, b2, scale, out[r:], None if out_lo is None else out_lo[r:])

    def conv12_pack(self, c1, c2, scale, sets=2, c3=None):
        """Repack the fused conv12 kernel's weight fragments of ``sets`` (bit 0 online, bit
        1 target; HIP backend only) -- after the target weights change; ``c3``: the fused
        conv3's too."""

    def conv12_fwd(self, ring, slots, frames_buf, scale, y1, y1_lo, y2, y2_lo, c1, c2, rows_first=0, copy_n=None,
                   pack_sets=3, c3=None, y3=None, y3_lo=None, y2_n=None):
        """conv1 -> conv2 in split mode: ``c1 = (w1 fp32, b1, w1 target, b1 target)``, ``c2 =
        (w2, w2_lo, b2, w2 target, w2_lo target, b2 target)`` (target entries None: one
        set).  y1 rows < ``copy_n`` must hold conv1's output afterwards (the backward's
        input); the HIP backend keeps the other rows in LDS (csrc/conv12_fused.hip) and
        repacks the weight fragments of ``pack_sets`` first (the others come from the last
        ``conv12_pack``).  ``c3 = (w3, w3_lo, b3, w3 target, w3_lo target, b3 target)``:
        conv3 too, into ``y3`` / ``y3_lo``; the HIP backend then writes y2 for rows <
        ``y2_n`` only (None: every row); this backend writes every row."""
        w1, b1, w1b, b1b = c1
        w2, w2l, b2, w2b, w2bl, b2b = c2
        self.conv1_fwd_ring(ring, slots, frames_buf, w1.to(y1.dtype), b1, scale, y1,
                            None if w1b is None else w1b.to(y1.dtype), b1b, rows_first, w32=w1, w2_32=w1b,
                            out_lo=y1_lo)
        self.conv_fwd(y1, w2, b2, 2, y2, w2b, b2b, rows_first, x_lo=y1_lo, w_lo=w2l, w2_lo=w2bl, out_lo=y2_lo)
        if c3 is not None:
            w3, w3l, b3, w3b, w3bl, b3b = c3
            self.conv_fwd(y2, w3, b3, 1, y3, w3b, b3b, rows_first, x_lo=y2_lo, w_lo=w3l, w2_lo=w3bl, out_lo=y3_lo)

    def conv_fwd(self, x, w, b, stride, out, w2=None, b2=None, rows_first=0, x_lo=None, w_lo=None, w2_lo=None,
                 out_lo=None):
        dt = torch.float32 if x_lo is not None else self.dtype
        xf = join(x, x_lo) if x_lo is not None else x
        if w2 is None:
            split_into(R.conv_fwd(xf, join(w, w_lo), b, stride, dt), out, out_lo)
        else:
            r = rows_first
            split_into(R.conv_fwd(xf[:r], join(w, w_lo), b, stride, dt), out[:r], None if out_lo is None else out_lo[:r])
            split_into(R.conv_fwd(xf[r:], join(w2, w2_lo), b2, stride, dt), out[r:],
                       None if out_lo is None else out_lo[r:])

    def fc_fwd(self, x, w, b, out, w2=None, b2=None, rows_first=0, x_lo=None, w_lo=None, w2_lo=None, out_lo=None,
               c2d=None, defer_head=False, ksplit=0):
        """``c2d = (conv2 weight, lo plane)``: weights of this step's conv2 data gradient,
        which the HIP backend pre-packs inside the fc launch; ``defer_head``: the HIP
        backend may leave the epilogue to the next :meth:`head` (both ignored here)."""
        dt = torch.float32 if x_lo is not None else self.dtype
        x = x.reshape(x.shape[0], -1)
        xf = join(x, x_lo.reshape(x.shape)) if x_lo is not None else x
        if w2 is None:
            split_into(R.fc_fwd(xf, join(w, w_lo), b, dt), out, out_lo)
        else:
            r = rows_first
            split_into(R.fc_fwd(xf[:r], join(w, w_lo), b, dt), out[:r], None if out_lo is None else out_lo[:r])
            split_into(R.fc_fwd(xf[r:], join(w2, w2_lo), b2, dt), out[r:], None if out_lo is None else out_lo[r:])

    # ---------------------------------------------------------------- head
    def head(self, Hon, Htg, Pon: Dict[str, torch.Tensor], Ptg: Dict[str, torch.Tensor], act, rew, gam, isw,
             huber: bool, kappa: float, grad_scale: float, td_abs, loss, dH, dhead, q_out=None,
             zero: Optional[torch.Tensor] = None, lo=None, isn=None, rescale_eps=None):
        """``rescale_eps`` (``Runtime.value_rescale``): the target is T = h(R + Gamma h^-1(q_target[a*])) of
        learner/rescale.py, fp64 on the fp32 values and rounded once (csrc/value_rescale.h).
        ``lo = (Hon_lo, Htg_lo, dH_lo)`` in split mode.  ``isn = (wscale, out[, count])``:
        batch-max IS normalisation, ``out[0] = max(isw) / wscale`` (the optimizer divides the
        gradient by it; csrc/ddqn_head.hip ``IsNorm``; ``out`` may be None), and ``count``
        (int64) += the rows with a non-zero weight (DP: the rows this rank drew)."""
        B = act.shape[0]
        dt = torch.float32
        lo = lo if lo is not None else (None, None, None)
        Hon, Htg = join(Hon, lo[0]), join(Htg, lo[1])
        q_t = self._dueling_q(Hon[:B], Pon, dt)
        q_n = self._dueling_q(Hon[B:2 * B], Pon, dt)
        q_g = self._dueling_q(Htg[:B], Ptg, dt)
        a_star = q_n.argmax(1)
        if rescale_eps is not None:
            G = rescale_target(rew.float().double(), gam.float().double(), q_g.gather(1, a_star[:, None]).squeeze(1).double(),
                               _lib.rescale_eps_arg(rescale_eps)).to(dt)
        else:
            G = rew.float() + gam.float() * q_g.gather(1, a_star[:, None]).squeeze(1)
        self._td_loss_bwd(G, q_t, Hon[:B], Pon, act, isw, huber, kappa, grad_scale, td_abs, loss, dH, dhead, q_out,
                          zero, lo[2], isn, dt)

    @staticmethod
    def _dueling_q(h, P, dt):
        """q [rows, A] of the scalar dueling head at stream activations ``h`` (stream width: 512 NatureCNN, 256
        IMPALA)."""
        HS = P["wv"].numel()
        v = h[:, :HS] @ P["wv"].to(dt) + P["bv"].to(dt)
        a = h[:, HS:] @ P["wa"].to(dt).t() + P["ba"].to(dt)
        return v[:, None] + a - a.mean(1, keepdim=True)

    def _td_loss_bwd(self, G, q_t, h, Pon, act, isw, huber, kappa, grad_scale, td_abs, loss, dH, dhead, q_out, zero,
                     dH_lo, isn, dt) -> None:
        """What :meth:`head` and :meth:`mdqn_head` share once the target ``G`` [B] stands: delta = G - q(S_t)[a],
        the Huber / squared loss, the priority, and the backward to ``dhead`` / ``dH`` (``h``: the online S_t
        rows)."""
        q_sa = q_t.gather(1, act.long()[:, None]).squeeze(1)
        delta = G - q_sa
        ad = delta.abs()
        if huber:
            lval = torch.where(ad <= kappa, 0.5 * delta * delta, kappa * (ad - 0.5 * kappa))
            dl = torch.where(ad <= kappa, delta, kappa * delta.sign())
        else:
            lval = 0.5 * delta * delta
            dl = delta
        w = isw.to(dt) if isw is not None else torch.ones_like(delta)
        dq = -w * dl * grad_scale
        td_abs.copy_(ad)
        loss.copy_(w * lval)
        self._dueling_bwd(dq[:, None], act, Pon, h, dH, dhead, dH_lo, dt)
        self._head_close(q_out, q_t, zero, isn, w)

    @staticmethod
    def _dhead(g, act, A: int, dhead, dt):
        """``dhead [B, (A + 1) N]`` from ``g [B, N]``, the gradient at the taken action's N outputs (N = 1: the
        scalar heads): the value rows get g, action a's rows g ([a = a_b] - 1/A).  Returns the advantage part
        ``[B, A, N]``."""
        B, N = g.shape
        onehot = torch.nn.functional.one_hot(act.long(), A).to(dt)
        dadv = g[:, None, :] * (onehot - 1.0 / A)[:, :, None]
        dhead[:, :N] = g
        dhead[:, N:] = dadv.reshape(B, A * N)
        return dadv

    def _dueling_bwd(self, g, act, Pon, h, dH, dhead, dH_lo, dt) -> None:
        """The dueling backward tail from ``g [B, N]`` (:meth:`_dhead`): ``dhead``, then through the head
        weights ``wv (N, HS)`` / ``wa (A N, HS)`` and the stream ReLUs of ``h`` to ``dH`` (+ ``dH_lo``)."""
        B, N = g.shape
        HS = Pon["wv"].shape[-1]
        A = Pon["wa"].shape[0] // N
        dadv = self._dhead(g, act, A, dhead, dt)
        wv = Pon["wv"].to(dt).reshape(N, HS)
        dv = g @ wv if N > 1 else g * wv       # (one value row: the plain product, no GEMM)
        da = dadv.reshape(B, A * N) @ Pon["wa"].to(dt)
        dh = torch.cat([dv, da], 1) * (h > 0).to(dt)
        split_into(dh, dH, dH_lo)

    def _head_close(self, q_out, q_t, zero, isn, w) -> None:
        """The heads' closing lines: ``q_out``, the zeroed head-gradient region, the IS statistic of ``w``."""
        if q_out is not None:
            q_out.copy_(q_t)
        if zero is not None:
            zero.zero_()
        self._is_norm_stats(isn, w)

    @staticmethod
    def _eps_greedy(q, eps, ctr, seed, q_out, a_out) -> None:
        """The actor heads' outputs: ``q_out`` and the epsilon-greedy action per row (host RNG seeded by
        ``seed`` and the counter)."""
        q_out.copy_(q)
        E, A = q_out.shape
        gen = torch.Generator(device="cpu").manual_seed(int(seed) * 1000003 + int(ctr.item()))
        u = torch.rand(E, generator=gen).to(q.device)
        r = torch.randint(0, A, (E,), generator=gen).to(q.device)
        a_out.copy_(torch.where(u < eps.to(q.device), r, q.argmax(1)).to(a_out.dtype))

    def mdqn_head(self, Hon, Htg, Pon: Dict[str, torch.Tensor], Ptg: Dict[str, torch.Tensor], act, rew, gam, isw,
                  huber: bool, kappa: float, alpha: float, tau: float, clip: float, grad_scale: float, td_abs, loss,
                  dH, dhead, q_out=None, aux=None, zero: Optional[torch.Tensor] = None, lo=None, isn=None):
        """The scalar head with the Munchausen-DQN target (csrc/mdqn_head.hip; learner/losses.py
        munchausen_loss is the definition).  ``Hon`` [B, 2 HS]: the online net at S_t; ``Htg`` [2B, 2 HS]:
        the target net, rows [0, B) at S_t+n (g1) and rows [B, 2B) at S_t (g0).  T = rew + alpha clamp(tau ln
        pi(a | g0), clip, 0) + gam (max g1 + tau ln sum exp((g1 - max g1) / tau)), delta = T - q_on[a]; loss,
        priority, ``dhead`` and ``dH`` as :meth:`head`.  ``aux`` [B, 2] fp32 (optional) receives (bonus, soft
        value) per row; ``lo``, ``zero`` and ``isn`` as :meth:`head`."""
        B = act.shape[0]
        assert Hon.shape[0] == B and Htg.shape[0] == 2 * B
        dt = _head_dtype(Hon)
        lo = lo if lo is not None else (None, None, None)
        Hon, Htg = join(Hon, lo[0], dt), join(Htg, lo[1], dt)
        q_t = self._dueling_q(Hon, Pon, dt)
        g1 = self._dueling_q(Htg[:B], Ptg, dt)
        g0 = self._dueling_q(Htg[B:], Ptg, dt)
        tau, alpha, clip = float(tau), float(alpha), float(clip)
        c0 = g0 - g0.max(1, keepdim=True).values
        tl0 = c0.gather(1, act.long()[:, None]).squeeze(1) - tau * torch.log(torch.exp(c0 / tau).sum(1))
        bonus = alpha * tl0.clamp(clip, 0.0)
        m1 = g1.max(1).values
        vsoft = m1 + tau * torch.log(torch.exp((g1 - m1[:, None]) / tau).sum(1))
        G = rew.to(dt) + bonus + gam.to(dt) * vsoft
        if aux is not None:
            aux[:, 0] = bonus
            aux[:, 1] = vsoft
        self._td_loss_bwd(G, q_t, Hon, Pon, act, isw, huber, kappa, grad_scale, td_abs, loss, dH, dhead, q_out, zero,
                          lo[2], isn, dt)

    @staticmethod
    def _is_norm_stats(isn, w) -> None:
        """The head's batch-max IS statistic (``isn`` of :meth:`head`) from the weights ``w``."""
        if isn is not None:
            if isn[1] is not None:   # tensor ops only: no host sync (graph-capturable)
                ws = isn[0].reshape(-1)[0].double() if isn[0] is not None else torch.ones((), dtype=torch.float64,
                                                                                           device=w.device)
                m = w.max().double()
                isn[1].reshape(-1)[0] = torch.where(ws > 0, m / torch.where(ws > 0, ws, torch.ones_like(ws)),
                                                    torch.zeros_like(m))
            if len(isn) > 2 and isn[2] is not None:
                isn[2].add_((w > 0).sum())

    # ------------------------------------------------- distributional (C51) head
    @staticmethod
    def _c51_logp(h, P, A: int, N: int, dt):
        """[rows, A, N] log-probabilities and [rows, A] expected q of stream activations ``h``:
        per-atom dueling combine, log-softmax over the atoms (max-subtracted)."""
        HS = P["wv"].shape[-1]
        v = h[:, :HS] @ P["wv"].to(dt).reshape(N, HS).t() + P["bv"].to(dt)
        a = (h[:, HS:] @ P["wa"].to(dt).t() + P["ba"].to(dt)).reshape(-1, A, N)
        return torch.log_softmax(v[:, None, :] + a - a.mean(1, keepdim=True), dim=-1)

    def c51_head(self, Hon, Htg, Pon: Dict[str, torch.Tensor], Ptg: Dict[str, torch.Tensor], act, rew, gam, isw,
                 num_atoms: int, v_min: float, v_max: float, grad_scale: float, td_abs, loss, dH, dhead,
                 q_out=None, zero: Optional[torch.Tensor] = None, lo=None, isn=None, rescale_eps=None):
        """The distributional counterpart of :meth:`head` (the oracle of csrc/c51_head.hip
        ``c51_head_kernel``): head weights ``wv (N, HS)``, ``bv (N,)``, ``wa (A N, HS)``, ``ba
        (A N,)``; loss = -w sum_i m_i log p(S_t)[a, i] with m the projected target
        distribution of the double-DQN action (learner/losses.py ``c51_project``), td_abs =
        |sum_i m_i z_i - q(S_t)[a]|, ``dhead [B, (A + 1) N]`` (value atoms, then action a's
        atoms at N + a N), ``q_out`` the expected q(S_t).  Computes in the head weights'
        dtype when that is fp64 (the tests' reference), else fp32."""
        def target(p_g, z):
            m = self._c51_m(p_g, rew, gam, v_min, v_max, rescale_eps)
            return m, (m * z).sum(-1)
        self._categorical_head(Hon, Htg, Pon, Ptg, act, isw, num_atoms, v_min, v_max, grad_scale, td_abs, loss, dH,
                               dhead, q_out, zero, lo, isn, target)

    def _dist_head(self, Hon, Htg, Pon, act, isw, num_atoms, td_abs, loss, dH, dhead, q_out, zero, lo, isn, rows):
        """What :meth:`c51_head`, :meth:`hlg_head` and :meth:`qr_head` share: the planes joined in the head's
        dtype, then ``rows(Hon, Htg, A, N, dt, ar, w)`` -> ``(q_t [B, A], td [B], loss [B], g [B, N])`` of the
        head (``ar`` = arange(B), ``w`` the IS weights or ones), then the outputs and the dueling backward."""
        B, N = act.shape[0], int(num_atoms)
        A = Pon["wa"].shape[0] // N
        dt = _head_dtype(Pon["wv"])
        lo = lo if lo is not None else (None, None, None)
        Hon, Htg = join(Hon, lo[0], dt), join(Htg, lo[1], dt)
        ar = torch.arange(B, device=Hon.device)
        w = isw.to(dt) if isw is not None else torch.ones(B, dtype=dt, device=Hon.device)
        q_t, td, loss_row, g = rows(Hon, Htg, A, N, dt, ar, w)
        td_abs.copy_(td)
        loss.copy_(loss_row)
        self._dueling_bwd(g, act, Pon, Hon[:B], dH, dhead, lo[2], dt)
        self._head_close(q_out, q_t, zero, isn, w.float())

    def _categorical_head(self, Hon, Htg, Pon, Ptg, act, isw, num_atoms, v_min, v_max, grad_scale, td_abs, loss, dH,
                          dhead, q_out, zero, lo, isn, target):
        """The categorical rows of :meth:`c51_head` and :meth:`hlg_head`: ``target(p_g, z)`` -> ``(m [B, N], ref
        [B])`` from the target net's distribution of the double-DQN action; loss = -w sum_i m_i log p(S_t)[a, i],
        td_abs = |ref - q(S_t)[a]|."""
        def rows(Hon, Htg, A, N, dt, ar, w):
            B = ar.shape[0]
            delta = (float(v_max) - float(v_min)) / (N - 1)
            z = float(v_min) + torch.arange(N, dtype=dt, device=Hon.device) * delta
            lp_t = self._c51_logp(Hon[:B], Pon, A, N, dt)
            q_t = (lp_t.exp() * z).sum(-1)
            a_star = (self._c51_logp(Hon[B:2 * B], Pon, A, N, dt).exp() * z).sum(-1).argmax(1)
            m, ref = target(self._c51_logp(Htg[:B], Ptg, A, N, dt)[ar, a_star].exp(), z)
            lp = lp_t[ar, act.long()]
            p = lp.exp()
            g = w[:, None] * (p - m) * grad_scale                      # d loss / d logits of (a_b, .)
            return q_t, (ref - (p * z).sum(-1)).abs(), -w * (m * lp).sum(-1), g
        self._dist_head(Hon, Htg, Pon, act, isw, num_atoms, td_abs, loss, dH, dhead, q_out, zero, lo, isn, rows)

    @staticmethod
    def _c51_m(p_g, rew, gam, v_min, v_max, rescale_eps):
        """The projected target distribution (learner/losses.py ``c51_project``).  With ``rescale_eps`` the moved
        atoms are formed as the kernel forms them: fp64 on the fp32 inputs, rounded to the head's dtype once."""
        from ..learner.losses import c51_project
        if rescale_eps is None:
            return c51_project(p_g, rew, gam, v_min, v_max)
        eps = _lib.rescale_eps_arg(rescale_eps)
        if p_g.dtype == torch.float64:
            return c51_project(p_g, rew, gam, v_min, v_max, eps)
        N, dt = p_g.shape[-1], p_g.dtype
        delta = (float(v_max) - float(v_min)) / (N - 1)
        idx = torch.arange(N, dtype=dt, device=p_g.device)
        z = float(v_min) + idx * delta
        tz = rescale_target(rew.to(dt).double()[:, None], gam.to(dt).double()[:, None], z.double()[None, :], eps).to(dt)
        b = (tz.clamp(float(v_min), float(v_max)) - float(v_min)) / delta
        m = torch.zeros_like(p_g)
        for j in range(N):
            m = m + p_g[:, j:j + 1] * (1.0 - (b[:, j:j + 1] - idx[None, :]).abs()).clamp_min(0.0)
        return m

    def hlg_head(self, Hon, Htg, Pon: Dict[str, torch.Tensor], Ptg: Dict[str, torch.Tensor], act, rew, gam, isw,
                 num_atoms: int, v_min: float, v_max: float, sigma_ratio: float, grad_scale: float, td_abs, loss, dH,
                 dhead, q_out=None, zero: Optional[torch.Tensor] = None, lo=None, isn=None, rescale_eps=None):
        """:meth:`c51_head` with the histogram-loss (HL-Gauss) target (the oracle of csrc/c51_head.hip
        ``hlg_head_kernel``): y = clamp(rew + gam q_target(S_t+n)[a*]) from the target net's expectation of the
        double-DQN action (with ``rescale_eps`` T(rew, gam, q_target[a*])), m its Gaussian mass per bin
        (learner/losses.py ``hl_gauss_target``: fp64 on y, rounded to the head's dtype once), loss = -w sum_i m_i
        log p(S_t)[a, i], td_abs = |y - q(S_t)[a]|; every output laid out as :meth:`c51_head`'s."""
        from ..learner.losses import hl_gauss_target

        def target(p_g, z):
            q_g = (p_g * z).sum(-1)
            if rescale_eps is None:
                y0 = rew.to(z.dtype) + gam.to(z.dtype) * q_g
            else:
                y0 = rescale_target(rew.to(z.dtype).double(), gam.to(z.dtype).double(), q_g.double(),
                                    _lib.rescale_eps_arg(rescale_eps)).to(z.dtype)
            y = y0.clamp(float(v_min), float(v_max))
            return hl_gauss_target(y, v_min, v_max, int(num_atoms), sigma_ratio), y
        self._categorical_head(Hon, Htg, Pon, Ptg, act, isw, num_atoms, v_min, v_max, grad_scale, td_abs, loss, dH,
                               dhead, q_out, zero, lo, isn, target)

    def c51_actor_head(self, H, P, eps, ctr, seed, num_atoms: int, v_min: float, v_max: float, q_out, a_out,
                       H_lo=None):
        """Expected q of the distributional head + epsilon-greedy per row (the oracle of
        csrc/c51_head.hip ``c51_actor_head_kernel``)."""
        N = int(num_atoms)
        dt = _head_dtype(P["wv"])
        h = join(H, H_lo, dt)
        delta = (float(v_max) - float(v_min)) / (N - 1)
        z = float(v_min) + torch.arange(N, dtype=dt, device=h.device) * delta
        q = (self._c51_logp(h, P, q_out.shape[1], N, dt).exp() * z).sum(-1)
        self._eps_greedy(q, eps, ctr, seed, q_out, a_out)

    # ------------------------------------------- quantile-regression (QR-DQN) head
    @staticmethod
    def _qr_theta(h, P, A: int, N: int, dt):
        """[rows, A, N] quantiles of stream activations ``h``: theta[a, i] = v[i] + adv[a, i] -
        mean_a' adv[a', i] (the dueling mean per quantile)."""
        HS = P["wv"].shape[-1]
        v = h[:, :HS] @ P["wv"].to(dt).reshape(N, HS).t() + P["bv"].to(dt)
        a = (h[:, HS:] @ P["wa"].to(dt).t() + P["ba"].to(dt)).reshape(-1, A, N)
        return v[:, None, :] + a - a.mean(1, keepdim=True)

    def qr_head(self, Hon, Htg, Pon: Dict[str, torch.Tensor], Ptg: Dict[str, torch.Tensor], act, rew, gam, isw,
                num_atoms: int, kappa: float, grad_scale: float, td_abs, loss, dH, dhead,
                q_out=None, zero: Optional[torch.Tensor] = None, lo=None, isn=None, rescale_eps=None):
        """The quantile-regression counterpart of :meth:`c51_head` (the oracle of
        csrc/qr_head.hip ``qr_head_kernel``), the same head weights read as N quantiles per
        action: T_j = R + Gamma theta_target(S_t+n)[a*, j] with a* the online net's double-DQN
        action (q = mean of the quantiles), loss = w sum_i rho_i and g = -w grad_scale c
        (learner/losses.py ``quantile_huber_terms``, kappa > 0), td_abs = |mean_j T_j -
        q(S_t)[a]|, ``dhead`` / ``dH`` / ``q_out`` laid out as :meth:`c51_head`'s.  Computes in
        the head weights' dtype when that is fp64 (the tests' reference), else fp32."""
        from ..learner.losses import quantile_huber_terms
        if not float(kappa) > 0.0:
            raise ValueError(f"qr_head: kappa must be > 0, got {kappa}")

        def rows(Hon, Htg, A, N, dt, ar, w):
            B = ar.shape[0]
            th_t = self._qr_theta(Hon[:B], Pon, A, N, dt)
            a_star = self._qr_theta(Hon[B:2 * B], Pon, A, N, dt).mean(-1).argmax(1)
            T = self._quantile_T(rew.to(dt), gam.to(dt), self._qr_theta(Htg[:B], Ptg, A, N, dt)[ar, a_star], rescale_eps)
            th = th_t[ar, act.long()]
            rho, c = quantile_huber_terms(th, T, kappa)
            g = -w[:, None] * grad_scale * c                           # d loss / d theta of (a_b, .)
            return th_t.mean(-1), (T.mean(-1) - th.mean(-1)).abs(), w * rho.sum(-1), g
        self._dist_head(Hon, Htg, Pon, act, isw, num_atoms, td_abs, loss, dH, dhead, q_out, zero, lo, isn, rows)

    @staticmethod
    def _quantile_T(rew, gam, theta, rescale_eps):
        """The target samples of the quantile heads (learner/losses.py ``quantile_targets``); with ``rescale_eps``
        in fp64 on the values of the head's dtype, rounded once (csrc/value_rescale.h)."""
        from ..learner.losses import quantile_targets
        if rescale_eps is None:
            return quantile_targets(rew, gam, theta)
        return quantile_targets(rew.double(), gam.double(), theta.double(), _lib.rescale_eps_arg(rescale_eps)).to(theta.dtype)

    def qr_actor_head(self, H, P, eps, ctr, seed, num_atoms: int, q_out, a_out, H_lo=None):
        """q = mean of the quantiles + epsilon-greedy per row (the oracle of csrc/qr_head.hip
        ``qr_actor_head_kernel``)."""
        N = int(num_atoms)
        dt = _head_dtype(P["wv"])
        q = self._qr_theta(join(H, H_lo, dt), P, q_out.shape[1], N, dt).mean(-1)
        self._eps_greedy(q, eps, ctr, seed, q_out, a_out)

    # ------------------------------------------------- implicit quantile (IQN) head
    @staticmethod
    def _iqn_theta(h, P, E, tau, dt):
        """theta [rows, A, n] and pre [rows, n, 2 HS] of stream activations ``h`` at the
        fractions ``tau`` [rows, n] (fp32): c = cos(pi i tau) (fp64 at the fp32 tau, then
        cast), pre = We c + be, x = h * relu(pre), v = wv . x[:HS] + bv, adv_a = wa[a] .
        x[HS:] + ba[a], theta[a] = v + adv_a - mean_a' adv_a'.  ``P``: the scalar head's
        shapes; ``E``: ``wtau (2 HS, 64)``, ``btau (2 HS,)``."""
        from ..learner.iqn import cos_features
        HS = P["wv"].shape[-1]
        cf = cos_features(tau, dt)
        pre = cf @ E["wtau"].to(dt).t() + E["btau"].to(dt)
        x = h[:, None, :] * torch.relu(pre)
        v = x[..., :HS] @ P["wv"].to(dt).reshape(HS) + P["bv"].to(dt).reshape(())
        adv = x[..., HS:] @ P["wa"].to(dt).t() + P["ba"].to(dt)
        th = v[..., None] + adv - adv.mean(-1, keepdim=True)
        return th.transpose(1, 2), pre, cf

    @staticmethod
    def iqn_workspace(B: int, N: int, device, dtype=torch.float32) -> Dict[str, torch.Tensor]:
        """What :meth:`iqn_head` leaves for :meth:`iqn_wgrad` (set 0 only): ``dpre [B, N, 2 HS]``,
        ``cos [B, N, 64]``, ``xg [B, 2 HS]`` = sum_k g_k x_k and ``gsum [B]`` = sum_k g_k."""
        z = lambda *s: torch.zeros(*s, device=device, dtype=dtype)      # noqa: E731
        return {"dpre": z(B, N, 1024), "cos": z(B, N, 64), "xg": z(B, 1024), "gsum": z(B)}

    @staticmethod
    def _iqn_update_index(ctr, base) -> int:
        u = int(ctr.reshape(-1)[0].item()) - (0 if base is None else int(base.reshape(-1)[0].item()))
        return max(u, 0)

    def iqn_head(self, Hon, Htg, Pon: Dict[str, torch.Tensor], Ptg: Dict[str, torch.Tensor],
                 Eon: Dict[str, torch.Tensor], Etg: Dict[str, torch.Tensor], act, rew, gam, isw, num_samples: int,
                 kappa: float, grad_scale: float, seed_q: int, ctr, base, td_abs, loss, dH, dhead, ws, q_out=None,
                 tau_out=None, zero: Optional[torch.Tensor] = None, lo=None, isn=None, max_blocks=None,
                 rescale_eps=None):
        """The implicit quantile counterpart of :meth:`qr_head` (the oracle of csrc/iqn_head.hip
        ``iqn_head_kernel``): the scalar head's weights ``P`` gated by the cosine embedding
        ``E`` (:meth:`_iqn_theta`) at three tau sets of N fractions per sample, drawn by the
        mirror learner/iqn.py ``learner_taus`` at update u = ctr - base: set 0 the online net at
        S_t, set 1 the online net at S_t+n (a* = first maximum of the mean), set 2 the target
        net at S_t+n (T_j).  loss, g, td_abs and ``dhead [B, (A + 1) N]`` as :meth:`qr_head`
        with tau_i of set 0; ``dH`` = [h > 0] sum_k phi_k dx_k; ``ws`` (:meth:`iqn_workspace`)
        receives what :meth:`iqn_wgrad` needs; ``tau_out [B, 3, N]`` the fractions used."""
        from ..learner.iqn import learner_taus
        from ..learner.losses import quantile_huber_terms
        B, N = act.shape[0], int(num_samples)
        A = Pon["wa"].shape[0]
        dt = _head_dtype(Pon["wv"])
        HS = Pon["wv"].shape[-1]
        if not float(kappa) > 0.0:
            raise ValueError(f"iqn_head: kappa must be > 0, got {kappa}")
        lo = lo if lo is not None else (None, None, None)
        Hon, Htg = join(Hon, lo[0], dt), join(Htg, lo[1], dt)
        taus = learner_taus(int(seed_q), self._iqn_update_index(ctr, base), B, N).to(Hon.device)
        if tau_out is not None:
            tau_out.copy_(taus)
        ar = torch.arange(B, device=Hon.device)
        th_t, pre, cf = self._iqn_theta(Hon[:B], Pon, Eon, taus[:, 0], dt)
        q_t = th_t.mean(-1)
        a_star = self._iqn_theta(Hon[B:2 * B], Pon, Eon, taus[:, 1], dt)[0].mean(-1).argmax(1)
        T = self._quantile_T(rew.to(dt), gam.to(dt), self._iqn_theta(Htg[:B], Ptg, Etg, taus[:, 2], dt)[0][ar, a_star],
                             rescale_eps)
        th = th_t[ar, act.long()]
        rho, c = quantile_huber_terms(th, T, kappa, taus[:, 0])
        w = isw.to(dt) if isw is not None else torch.ones(B, dtype=dt, device=Hon.device)
        td_abs.copy_((T.mean(-1) - th.mean(-1)).abs())
        loss.copy_(w * rho.sum(-1))
        g = -w[:, None] * grad_scale * c                           # d loss / d theta of (a_b, .)
        dadv = self._dhead(g, act, A, dhead, dt)                    # [B, A, N]
        # back through the heads, the gate and the stream ReLUs
        dxv = g[:, :, None] * Pon["wv"].to(dt).reshape(HS)          # [B, N, HS]
        dxa = torch.einsum("bak,ac->bkc", dadv, Pon["wa"].to(dt))
        dx = torch.cat([dxv, dxa], -1)
        phi = torch.relu(pre)
        h = Hon[:B]
        dh = (phi * dx).sum(1) * (h > 0).to(dt)
        split_into(dh, dH, lo[2])
        ws["dpre"].copy_((pre > 0).to(dt) * dx * h[:, None, :])
        ws["cos"].copy_(cf)
        ws["xg"].copy_((g[:, :, None] * (h[:, None, :] * phi)).sum(1))
        ws["gsum"].copy_(g.sum(1))
        self._head_close(q_out, q_t, zero, isn, w.float())

    def iqn_wgrad(self, act, ws, g: Dict[str, torch.Tensor], prio=None) -> None:
        """The head and embedding weight gradients from what :meth:`iqn_head` left (the oracle of
        csrc/iqn_wgrad.h ``iqn_wgrad_body``); written, not accumulated.  ``prio = (replay, idx, gen,
        td_abs)``: also write the batch's priorities back (the HIP backend: one block of the same launch).
        G[wv] = sum_b xg_b[:HS], G[wa][a] = sum_b ([a = a_b] - 1/A) xg_b[HS:], G[bv] = sum_b
        gsum_b, G[ba][a] = sum_b ([a = a_b] - 1/A) gsum_b, G[btau] = sum_{b,k} dpre, G[wtau] =
        sum_{b,k} dpre (x) cos."""
        if prio is not None:
            prio[0].update_priorities(prio[1], prio[3], prio[2])
        dt = g["wa"].dtype
        A, HS = g["wa"].shape
        coef = torch.nn.functional.one_hot(act.long(), A).to(dt) - 1.0 / A
        xg, gs = ws["xg"].to(dt), ws["gsum"].to(dt)
        g["wv"].copy_(xg[:, :HS].sum(0).reshape(g["wv"].shape))
        g["bv"].copy_(gs.sum().reshape(g["bv"].shape))
        g["wa"].copy_(coef.t() @ xg[:, HS:])
        g["ba"].copy_(coef.t() @ gs)
        g["btau"].copy_(ws["dpre"].to(dt).sum((0, 1)))
        g["wtau"].copy_(torch.einsum("bkc,bki->ci", ws["dpre"].to(dt), ws["cos"].to(dt)))

    def iqn_actor_head(self, H, P, E, eps, ctr, seed, seed_q, tau_ctr, stream: int, num_samples: int,
                       midpoint: bool, q_out, a_out, H_lo=None, tau_out=None):
        """q = the mean of theta over K fractions per env row + epsilon-greedy (the oracle of
        csrc/iqn_head.hip ``iqn_actor_head_kernel``): fractions of the counter word 64
        tau_ctr + stream (learner/iqn.py ``stream_taus``), or the midpoints."""
        from ..learner.iqn import midpoint_taus, stream_taus
        K = int(num_samples)
        dt = _head_dtype(P["wv"])
        h = join(H, H_lo, dt)
        n_e = q_out.shape[0]
        if midpoint:
            taus = midpoint_taus(K).to(h.device)[None, :].expand(n_e, K).contiguous()
        else:
            taus = stream_taus(int(seed_q), 64 * int(tau_ctr.reshape(-1)[0].item()) + int(stream), n_e, K).to(h.device)
        if tau_out is not None:
            tau_out.copy_(taus)
        q = self._iqn_theta(h, P, E, taus, dt)[0].mean(-1)
        self._eps_greedy(q, eps, ctr, seed, q_out, a_out)

    def head_wgrad(self, Hon, dhead, g: Dict[str, torch.Tensor], prio=None, Hon_lo=None, pack=None):
        """``prio = (replay, idx, gen, td_abs)``: also write the batch's priorities back
        (the HIP backend runs it as one extra block of the same launch).  ``pack = (dst,
        segs)``: also the :meth:`pack_rows` of the DP step's factor rows (HIP: tail blocks
        of the same launch).  ``g["wv"]`` of shape (N, HS): N value rows (the distributional
        head; ``dhead [B, N + A N]``)."""
        if pack is not None:
            self.pack_rows(*pack)
        if prio is not None:
            prio[0].update_priorities(prio[1], prio[3], prio[2])
        B = dhead.shape[0]
        if g["wv"].dim() == 2:
            NV, HS = g["wv"].shape
            dt = g["wv"].dtype
            h = Hon[:B].to(dt) if Hon_lo is None else Hon[:B].to(dt) + Hon_lo[:B].to(dt)
            dh = dhead.to(dt)
            g["wv"].add_(dh[:, :NV].t() @ h[:, :HS])
            g["bv"].add_(dh[:, :NV].sum(0))
            g["wa"].add_(dh[:, NV:].t() @ h[:, HS:])
            g["ba"].add_(dh[:, NV:].sum(0))
            return
        HS = g["wv"].numel()
        h = join(Hon[:B], None if Hon_lo is None else Hon_lo[:B])
        g["wv"].add_(dhead[:, 0] @ h[:, :HS])
        g["bv"].add_(dhead[:, 0].sum().view(1))
        g["wa"].add_(dhead[:, 1:].t() @ h[:, HS:])
        g["ba"].add_(dhead[:, 1:].sum(0))

    def actor_head(self, H, P, eps, ctr, seed, q_out, a_out, H_lo=None):
        """Dueling q + epsilon-greedy per row (the oracle of csrc actor_head_kernel);
        ``H_lo``: split mode, the activations' lo plane."""
        q = self._dueling_q(join(H, H_lo), P, torch.float32)
        self._eps_greedy(q, eps, ctr, seed, q_out, a_out)

    # ------------------------------------------------------------ backward
    def fc_bwd(self, dh, x, w, dx_out, dw_out, db_out):
        self.fc_dgrad(dh, x, w, dx_out)
        self.fc_wgrad(dh, x, dw_out, db_out)

    def fc_dgrad(self, dh, x, w, dx_out, dh_lo=None, w_lo=None, dx_lo=None):
        """dx = (dh @ w) * (x > 0) (x = the ReLU'd fc input)."""
        xf = x.reshape(x.shape[0], -1)
        if dh_lo is not None:
            dx = (join(dh, dh_lo) @ join(w, w_lo)) * (xf > 0).float()
            split_into(dx, dx_out, dx_lo)
            return
        dx, _, _ = R.fc_bwd(dh, xf, w, xf, self.dtype)
        dx_out.copy_(dx.reshape(dx_out.shape))

    def fc_wgrad(self, dh, x, dw_out, db_out, norm=None, dh_lo=None, x_lo=None):
        """``norm = (partials, slot0)``: also the squared norm of what it writes, in fp64
        at ``partials[slot0]`` (one slot; the HIP kernel writes 4 per workgroup)."""
        xf = join(x.reshape(x.shape[0], -1), None if x_lo is None else x_lo.reshape(x.shape[0], -1))
        dhf = join(dh, dh_lo)
        dw_out.copy_(dhf.t() @ xf)
        db_out.copy_(dhf.sum(0))
        if norm is None:
            return 0
        part, s0 = norm
        part[s0] = dw_out.double().pow(2).sum() + db_out.double().pow(2).sum()
        return 1

    def fc_wgrad_split(self, dh, x, dw_out, db_out, jobs, split_rows: int, jnorm, dh_lo=None, x_lo=None,
                       cpb: int = -1) -> int:
        """The fc weight gradient as split-K partials reduced by the step's
        ``finalize_grads`` (HIP: a job appended to ``jobs``); its squared-norm partials go
        to ``jnorm`` (one per finalize block).  Returns the partial count.  The torch
        path computes it at once (one partial)."""
        return self.fc_wgrad(dh, x, dw_out, db_out, norm=(jnorm, 0), dh_lo=dh_lo, x_lo=x_lo)

    def fc_head_wgrad(self, dh, x, dw_out, db_out, Hon, dhead, g_head, prio, norm=None, dh_lo=None, x_lo=None,
                      Hon_lo=None) -> int:
        """fc weight gradient + head weight gradient (+ the priority write-back,
        ``prio = (replay, idx, gen, td_abs)``); returns the fc norm slots used."""
        self.head_wgrad(Hon, dhead, g_head, prio=prio, Hon_lo=Hon_lo)
        return self.fc_wgrad(dh, x, dw_out, db_out, norm=norm, dh_lo=dh_lo, x_lo=x_lo) or 0

    def finalize_grads(self, jobs, norm_range=None, norm=None) -> int:
        """Deferred split-K reductions (the torch path computes gradients directly)."""
        return 0

    def conv_dgrad(self, dy, w, stride, x_src, dx_out, dy_lo=None, w_lo=None, dx_lo=None):
        if dy_lo is not None:
            dx = R.conv_dgrad(join(dy, dy_lo), join(w, w_lo), tuple(x_src.shape), stride, x_src, torch.float32)
            split_into(dx, dx_out, dx_lo)
            return
        dx_out.copy_(R.conv_dgrad(dy, w, tuple(x_src.shape), stride, x_src, self.dtype))

    def conv_wgrad(self, dy, x, k, stride, dw_out, db_out, jobs=None, dy_lo=None, x_lo=None):
        dw, db = R.conv_wgrad(join(dy, dy_lo), join(x, x_lo), k, stride)
        dw_out.copy_(dw)
        db_out.copy_(db)

    def conv1_wgrad(self, dy, frames, scale, dw_out, db_out, dy_lo=None):
        dw, db = R.conv1_wgrad(join(dy, dy_lo), frames, scale)
        dw_out.copy_(dw)
        db_out.copy_(db)

    def conv1_wgrad_ring(self, dy, ring, slots, frames_buf, scale, dw_out, db_out, jobs=None, dy_lo=None):
        self.conv1_wgrad(dy, frames_buf[:slots.shape[0]], scale, dw_out, db_out, dy_lo=dy_lo)

    def conv21_fused_ok(self, dy2, slots, dy2_lo=None, w2_lo=None) -> bool:
        """Whether :meth:`conv2_dgrad_conv1_wgrad` runs as one fused kernel for these arguments."""
        return False

    def conv2_dgrad_conv1_wgrad(self, dy2, w2, y1, dy1, ring, slots, frames_buf, scale, dw_out, db_out, jobs=None,
                                dy2_lo=None, w2_lo=None, dy1_lo=None):
        """conv2's data gradient (dY2 -> dY1, masked by y1) followed by conv1's weight gradient
        on dY1 -- the arguments of :meth:`conv_dgrad` and :meth:`conv1_wgrad_ring`.  Here the
        two calls; the HIP backend fuses them where it can (then ``dy1`` is not written)."""
        self.conv_dgrad(dy2, w2, 2, y1, dy1, dy_lo=dy2_lo, w_lo=w2_lo, dx_lo=dy1_lo)
        self.conv1_wgrad_ring(dy1, ring, slots, frames_buf, scale, dw_out, db_out, jobs=jobs, dy_lo=dy1_lo)

    # ----------------------------------------------------------- optimizer
    def optimizer(self, p32, g32, v, m, pbf, lr, alpha, eps, clip, centered, partials, norm_out, norm_total=None,
                  sample=None, pb_lo=None, wnorm=None, frag_out=None, segs=None, norm_prefix=None, opt=None,
                  target=None):
        """``sample = (replay, B, out, nxt2[, obs2])``: also draw the next
        batch after the update (the HIP backend fuses it into the optimizer launch; ``obs2``: the
        sampler's second copy of the S_t slots, the Munchausen row plan).
        ``pb_lo``: split mode, the lo plane of the bf16 copy.  ``wnorm = (stats, n,
        stride)``: batch-max IS normalisation, the gradient is divided by the largest of
        the n per-rank maxima ``stats[k * stride]`` (csrc/rmsprop_common.h is_grad_scale).
        ``norm_total = (partials, n)``: the clip norm is sqrt(sum(partials[:n])) (squared-norm
        partials written by the gradient producers) instead of a pass over ``g32``.
        ``segs``: [(offset, length), ...] -- update only these ranges of the flat arrays
        (the sharded data-parallel update; needs ``norm_total``).  ``norm_prefix``: a
        gradient range whose squares join the partials' sum (summed inside the launch).
        ``opt`` (learner/schedules.py ``OptSpec``): Adam instead of RMSprop (``v`` / ``m`` hold
        the second / first moment; ``alpha``, ``eps`` and ``centered`` are unused) and / or
        the step-indexed learning rate, both from the update index on the device.
        ``target = (t32, tbf, tbf_lo, rho, frag_out_target)``: the soft target net averaged with the
        weights just written, t <- (1 - rho) t + rho p (learner/schedules.py ``target_ema``), and its
        bf16 planes; ``frag_out_target``: the fused forward's target fragments too (HIP backend)."""
        self._optimizer(p32, g32, v, m, pbf, lr, alpha, eps, clip, centered, norm_out, pb_lo, wnorm, norm_total,
                        segs, norm_prefix, opt)
        if target is not None:
            if segs is not None:
                raise ValueError("the soft target is averaged over the whole parameter vector, not in a sharded update")
            self._target_ema(p32, *target[:4])
        if sample is not None:
            rp, B, out, nxt2, obs2 = _sample5(sample)
            rp.sample(B, out=out, nxt2=nxt2, **({} if obs2 is None else {"obs2": obs2}))

    def _optimizer(self, p32, g32, v, m, pbf, lr, alpha, eps, clip, centered, norm_out, pb_lo=None, wnorm=None,
                   norm_total=None, segs=None, norm_prefix=None, opt=None):
        sc = torch.ones((), dtype=torch.float32, device=g32.device)
        adam = opt is not None and opt.adam
        if opt is not None:       # tensor ops only: the index is read on the device
            lr = opt.lr_tensor().to(g32.device)
        if adam:
            c1, c2 = (c.to(g32.device) for c in opt.corrections())
            b1, b2 = float(np.float32(opt.beta1)), float(np.float32(opt.beta2))
            d1, d2 = float(np.float32(1) - np.float32(opt.beta1)), float(np.float32(1) - np.float32(opt.beta2))
        if wnorm is not None:     # tensor ops only: no host sync (graph-capturable)
            st, n, stride = wnorm
            mx = st.reshape(-1)[0:n * stride:stride].max().float()
            sc = torch.where(mx > 0, 1.0 / mx.clamp_min(1e-30), sc)
        if norm_total is not None:
            part, npart = norm_total if isinstance(norm_total, tuple) else (norm_total, 1)
            sq = part[:npart].double().sum()
            if norm_prefix is not None:
                sq = sq + norm_prefix.double().pow(2).sum()
        else:
            assert segs is None, "a sharded update needs the clip norm's partials (norm_total)"
            sq = g32.double().pow(2).sum()
        norm = sq.sqrt().float() * sc
        coef = torch.clamp(clip / (norm + 1e-6), max=1.0) if clip > 0 else torch.ones_like(norm)
        for o, n in (segs if segs is not None else [(0, p32.numel())]):
            r = slice(o, o + n)
            g = g32[r] * (coef * sc)
            vr, mr, pr = v[r], m[r], p32[r]
            if adam:
                mr.mul_(b1).add_(d1 * g)
                vr.mul_(b2).add_(d2 * g * g)
                pr.sub_(lr * (mr / c1) / ((vr / c2).sqrt() + opt.adam_eps))
                split_into(pr, pbf[r], None if pb_lo is None else pb_lo[r])
                continue
            vr.mul_(alpha).add_((1 - alpha) * g * g)
            if centered:
                mr.mul_(alpha).add_((1 - alpha) * g)
                var = vr - mr * mr
            else:
                var = vr
            pr.sub_(lr * g / (var.clamp_min(0).sqrt() + eps))
            split_into(pr, pbf[r], None if pb_lo is None else pb_lo[r])
        norm_out.copy_(norm.view(1))

    @staticmethod
    def _target_ema(p32, t32, tbf, tbf_lo, rho) -> None:
        """The mirror's three roundings as separate fp32 tensor operations (no addcmul / lerp)."""
        r = torch.tensor(float(rho), dtype=torch.float32, device=p32.device)
        a = torch.ones_like(r) - r
        ta = t32 * a
        pr = p32 * r
        torch.add(ta, pr, out=t32)
        split_into(t32, tbf, tbf_lo)

    def gather_frames(self, replay, slots, out):
        replay.gather_frames(slots, out)

    # ------------------------------------------------------- noisy layers
    def noisy_compose(self, plan, nets, xi, fc32=None, xi_in=None) -> None:
        """Effective parameters of the noisy fc and head layers (learner/noisy.py; the oracle of
        csrc/noisy.hip ``noisy_compose_kernel``).  ``plan``: a ``NoisyPlan``; ``nets``: [(flat
        parameters with mu and sigma segments, fp32 shadow, bf16 shadow hi, lo or None), ...],
        net i drawing with stream ``plan.stream0 + i`` at the index ``plan.index()``; the shadows
        have the mu layout and get W = mu + sigma (xi_out (x) xi_in), evaluated in fp64 and
        rounded to fp32: heads and noisy biases into the fp32 shadow, ``wfc`` split into hi (+
        lo).  ``xi`` [len(nets), >= K] receives the draws (fp32, which is what enters W);
        ``fc32``: per net an optional (1024, 3136) fp32 output of the effective ``wfc``;
        ``xi_in`` (tests): these draws instead of the mirror's."""
        from ..learner import noisy as NZ
        K = plan.K
        u = plan.index() if xi_in is None else 0
        for i, (p, e32, ehi, elo) in enumerate(nets):
            if xi_in is None:
                xi[i, :K].copy_(NZ.noise_vectors(plan.seed, u, plan.stream0 + i, plan.A, plan.N)["xi"])
            else:
                xi[i, :K].copy_(xi_in[i, :K])
            v = NZ.split_xi(xi[i].double(), plan.A, plan.N)
            for name in NZ.MU:
                mu = plan.seg(p, name).double()
                w = (mu + plan.seg(p, NZ.SIGMA[name]).double() * NZ.outer(v, name, mu.shape).to(mu.device)).float()
                if name == "wfc":
                    split_into(w, plan.seg(ehi, name), None if elo is None else plan.seg(elo, name))
                    if fc32 is not None and fc32[i] is not None:
                        fc32[i].copy_(w)
                else:
                    plan.seg(e32, name).copy_(w)

    def noisy_sigma_grad(self, plan, g32, xi) -> None:
        """G[sigma] = G[mu] * xi_out (x) xi_in for the six noisy segments of the flat gradient,
        from the draw ``xi`` (K values, the online net's); the product in fp64, rounded once
        (the oracle of csrc/noisy.hip ``noisy_sigma_grad_kernel``)."""
        from ..learner import noisy as NZ
        v = NZ.split_xi(xi.reshape(-1).double(), plan.A, plan.N)
        for name in NZ.MU:
            gm = plan.seg(g32, name).double()
            plan.seg(g32, NZ.SIGMA[name]).copy_((gm * NZ.outer(v, name, gm.shape).to(gm.device)).float())

    # ------------------------------------------------- frame augmentation
    @staticmethod
    def _augment_check(ring, slots, pad, ctr, base, out, off_out):
        rows, C = slots.shape
        assert ring.dtype == torch.uint8 and ring.is_contiguous() and tuple(ring.shape[1:]) == (84, 84)
        assert slots.dtype == torch.int32 and slots.is_contiguous()
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= rows * C * 7056
        assert off_out.dtype == torch.int32 and off_out.is_contiguous() and off_out.numel() >= 2 * rows
        assert ctr.dtype == torch.int64 and (base is None or base.dtype == torch.int64)
        return int(rows), int(C)

    def augment_shift(self, ring, slots, pad, seed, ctr, base, out, off_out) -> None:
        """Random-shift augmentation of the frame stacks ``slots`` [rows, C] name in ``ring`` (learner/augment.py;
        the oracle of csrc/augment.hip ``augment_shift_kernel``): ``out`` gets the rows C shifted frames in the
        ring's space-to-depth layout, ``off_out`` [rows, 2] the offsets, drawn with ``seed`` (seed_a) at the update
        index ``ctr - base`` read back from the device."""
        from ..learner import augment as AU
        from ..replay.gpu_replay import from_s2d, to_s2d
        rows, C = self._augment_check(ring, slots, pad, ctr, base, out, off_out)
        u = max(int(ctr.reshape(-1)[0].item()) - (0 if base is None else int(base.reshape(-1)[0].item())), 0)
        off = AU.shift_offsets(seed, u, rows, pad)
        nat = from_s2d(ring[slots.long()].reshape(rows * C, 84, 84)).reshape(rows, C, 84, 84)
        sh = AU.shift_frames(nat, off, pad)
        out.reshape(-1)[:rows * C * 7056].copy_(to_s2d(sh.reshape(rows * C, 84, 84)).reshape(-1))
        off_out.reshape(-1)[:2 * rows].copy_(off.reshape(-1))

    # ------------------------------------------------------ periodic resets
    @staticmethod
    def _reset_check(table, p32, t32, v, m, pb, tb) -> int:
        from ..learner import reset as RS
        n = int(p32.numel())
        for t in (p32, t32, v, m):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
        for hi, lo in (pb, tb):
            assert hi.is_contiguous() and hi.numel() == n and (lo is None or (lo.is_contiguous() and lo.numel() == n
                                                                              and lo.dtype == hi.dtype))
        assert pb[0].dtype == tb[0].dtype and len(table) <= RS.MAX_ROWS
        return n

    def reset_perturb(self, table, seed, r, p32, t32, v, m, pb, tb) -> None:
        """Shrink-and-perturb reset ``r`` of the flat parameters (learner/reset.py ``apply_reset``; the oracle of
        csrc/reset.hip ``reset_perturb_kernel``): ``p32`` / ``t32`` mixed with the fresh values of ``table`` drawn
        with ``seed`` (seed_r), the moments ``v`` / ``m`` zeroed, and the bf16 planes ``pb`` = (hi, lo or None),
        ``tb`` of both nets rewritten from the result -- inside the table's rows only."""
        from ..learner import reset as RS
        self._reset_check(table, p32, t32, v, m, pb, tb)
        arrs = [t.detach().cpu().numpy().copy() for t in (p32, t32, v, m)]
        RS.apply_reset(*arrs, int(seed), int(r), table)
        for row in table:
            s = slice(row.start, row.end)
            for t, a in zip((p32, t32, v, m), arrs):
                t[s].copy_(torch.from_numpy(a[s]))
            for src, (hi, lo) in ((p32, pb), (t32, tb)):
                split_into(src[s], hi[s], None if lo is None else lo[s])

    # ------------------------------------------- data-parallel gradient factors
    def pack_rows(self, dst: torch.Tensor, segs) -> None:
        """dst[:, c0:c0 + n] = seg for the 2-D ``segs`` laid side by side (same row count)."""
        c0 = 0
        for t in segs:
            t2 = t.reshape(t.shape[0], -1)
            dst[:t2.shape[0], c0:c0 + t2.shape[1]].copy_(t2)
            c0 += t2.shape[1]

    def sqnorm_ranges(self, ranges, partials: torch.Tensor, nblk: int) -> int:
        """Squared-norm partials of the fp32 ``ranges`` into ``partials`` (fp64; the HIP
        kernel writes ``nblk`` block partials, this one slot).  Returns the slots written."""
        partials[0] = sum(r.double().pow(2).sum() for r in ranges if r is not None)
        return 1


class HipBackend(TorchBackend):
    """MI355X backend: the hand-written gfx950 kernels (``kernels`` lists the op
    families).  A missing kernel library is an error (``_lib.require_kernels``)."""

    name = "hip"

    def __init__(self, dtype=torch.bfloat16, native_conv: bool = True):
        super().__init__(dtype)
        self.lib = _lib.require_kernels()
        self.native_conv = native_conv and hasattr(self.lib, "apex_conv_fwd")
        self.kernels = ["replay", "head", "head_wgrad", "optimizer", "actor_head", "c51_head", "c51_actor_head", "qr_head",
                        "qr_actor_head", "noisy_compose", "noisy_sigma_grad", "mdqn_head", "iqn_head", "iqn_wgrad",
                        "iqn_actor_head", "augment_shift", "hlg_head", "reset_perturb"]
        if self.native_conv:
            self.kernels += ["conv_fwd", "conv_dgrad", "conv_wgrad", "fc_fwd", "fc_bwd"]
        self.ws = C.Workspace()

    # --------------------------------------------------- native conv family
    def conv1_fwd_ring(self, ring, slots, frames_buf, w, b, scale, out, w2=None, b2=None, rows_first=0, w32=None,
                       w2_32=None, out_lo=None, c2f=None):
        if not self.native_conv:
            return super().conv1_fwd_ring(ring, slots, frames_buf, w, b, scale, out, w2, b2, rows_first, w32, w2_32,
                                          out_lo)
        c2f = c2f if (c2f is not None and SW.c2f_pack) else None
        C.conv1_s2d_fwd(self.lib, self.ws, ring, slots, w, b, scale, out, w2, b2, rows_first, w32=w32, w2_32=w2_32,
                        out_lo=out_lo, c2f=c2f)
        if c2f is not None:   # this step's split conv2 forward finds its weights packed
            self._c2f_packed = tuple(_lib.ptr(t) for t in c2f)

    def _conv12_native(self) -> bool:
        return self.native_conv and SW.conv12_fused and hasattr(self.lib, "apex_conv12_fused_fwd")

    def conv12_pack(self, c1, c2, scale, sets=2, c3=None):
        if not self._conv12_native():
            return
        w1, b1, w1b, b1b = c1
        w2, w2l, b2, w2b, w2bl, b2b = c2
        C.conv12_pack(self.lib, self.ws, w1, b1, w2, w2l, b2, scale, w1b=w1b, b1b=b1b, w2b=w2b, w2b_lo=w2bl,
                      b2b=b2b, sets=sets, c3=c3)

    def conv12_fwd(self, ring, slots, frames_buf, scale, y1, y1_lo, y2, y2_lo, c1, c2, rows_first=0, copy_n=None,
                   pack_sets=3, c3=None, y3=None, y3_lo=None, y2_n=None):
        if not self._conv12_native():
            return super().conv12_fwd(ring, slots, frames_buf, scale, y1, y1_lo, y2, y2_lo, c1, c2, rows_first,
                                      copy_n, c3=c3, y3=y3, y3_lo=y3_lo)
        w1, b1, w1b, b1b = c1
        w2, w2l, b2, w2b, w2bl, b2b = c2
        n = slots.shape[0] if copy_n is None else int(copy_n)
        C.conv12_fused_fwd(self.lib, self.ws, ring, slots, w1, b1, w2, w2l, b2, scale, y2, y2_lo, y1=y1, y1_lo=y1_lo,
                           copy_n=n, w1b=w1b, b1b=b1b, w2b=w2b, w2b_lo=w2bl, b2b=b2b, rows_first=rows_first,
                           pack_sets=pack_sets, c3=c3, y3=y3, y3_lo=y3_lo, y2_n=y2_n)

    def conv_fwd(self, x, w, b, stride, out, w2=None, b2=None, rows_first=0, x_lo=None, w_lo=None, w2_lo=None,
                 out_lo=None):
        if not self.native_conv:
            return super().conv_fwd(x, w, b, stride, out, w2, b2, rows_first, x_lo, w_lo, w2_lo, out_lo)
        key = (_lib.ptr(w), _lib.ptr(w_lo), _lib.ptr(w2), _lib.ptr(w2_lo))
        packed = stride == 2 and getattr(self, "_c2f_packed", None) == key
        if packed:
            self._c2f_packed = None
        C.conv_fwd(self.lib, x, w, b, stride, out, w2, b2, rows_first, x_lo=x_lo, w_lo=w_lo, w2_lo=w2_lo,
                   out_lo=out_lo, packed=packed)

    def fc_fwd(self, x, w, b, out, w2=None, b2=None, rows_first=0, x_lo=None, w_lo=None, w2_lo=None, out_lo=None,
               c2d=None, defer_head=False, ksplit=0):
        """``ksplit`` > 0: that K split instead of the one that fills the chip (the actors:
        a throughput job beside the learner, where fewer partial planes cost less)."""
        if not self.native_conv:
            return super().fc_fwd(x, w, b, out, w2, b2, rows_first, x_lo, w_lo, w2_lo, out_lo)
        M, K = x.shape[0], x[0].numel()
        if w.shape[0] % 128 == 0 and K % 64 == 0 and hasattr(self.lib, "apex_fc_gemm128"):
            # 128x128 tiles, K split in two, loader waves: fc forward 40.6 -> 36.2 us
            # (split) / 25.7 -> 22.5 (bf16) at the learner shape (scripts/bench_fc128.py)
            defer = defer_head and w2 is not None and b is not None and b2 is not None and \
                2 * (M // 3) == rows_first and M % 3 == 0
            # K splits so the launch fills the chip: 2 at the learner's 1536 rows (96 tiles,
            # 192 blocks), more for the few row tiles of a small per-rank batch (global-batch
            # DP: 74 rows per rank -> 24 tiles x 10 splits)
            tiles = C.row_tiles_host(M, rows_first if w2 is not None else None, 128) * (w.shape[0] // 128)
            if ksplit > 0:
                ks = int(ksplit)
            else:
                ks = max(2, 256 // max(tiles, 1))
                if SW.fc_ksplit_max > 0:
                    ks = max(1, min(ks, SW.fc_ksplit_max))
            r = C.dense_fwd128(self.lib, self.ws, x.reshape(M, K), w, b, out, True, w2, b2, rows_first, ks, True,
                               x_lo=None if x_lo is None else x_lo.reshape(M, K), w_lo=w_lo, w2_lo=w2_lo,
                               out_lo=out_lo, c2d_pack=None if defer else c2d, no_epilogue=defer)
            if defer:
                # the split-K epilogue (and the conv2 pack) move into the next head launch
                self._fc_part = dict(part=r[0], nz=r[1], zstride=M * w.shape[0], b=b, b2=b2,
                                     two_b=rows_first, out=out, c2d=c2d)
                return
            # the conv2 data gradient of this step finds its weights packed (the key is
            # checked there, so a different weight tensor still packs its own)
            if c2d is not None:
                self._c2d_packed = (c2d[0].data_ptr(), _lib.ptr(c2d[1]))
            return
        C.dense_fwd(self.lib, x.reshape(x.shape[0], -1), w, b, out, relu=True, w2=w2, b2=b2,
                    rows_first=rows_first, ws=self.ws,
                    x_lo=None if x_lo is None else x_lo.reshape(x.shape[0], -1), w_lo=w_lo, w2_lo=w2_lo,
                    out_lo=out_lo)

    def fc_dgrad(self, dh, x, w, dx_out, dh_lo=None, w_lo=None, dx_lo=None):
        if not self.native_conv:
            return super().fc_dgrad(dh, x, w, dx_out, dh_lo, w_lo, dx_lo)
        xf = x.reshape(x.shape[0], -1)
        C.dense_dgrad(self.lib, dh, w, dx_out.reshape(dh.shape[0], -1), xf, dh_lo=dh_lo, w_lo=w_lo,
                      out_lo=None if dx_lo is None else dx_lo.reshape(dh.shape[0], -1))

    def fc_wgrad(self, dh, x, dw_out, db_out, norm=None, dh_lo=None, x_lo=None):
        if not self.native_conv:
            return super().fc_wgrad(dh, x, dw_out, db_out, dh_lo=dh_lo, x_lo=x_lo)
        return C.dense_wgrad(self.lib, dh, x.reshape(x.shape[0], -1), dw_out, db_out, norm=norm, dy_lo=dh_lo,
                             x_lo=None if x_lo is None else x_lo.reshape(x.shape[0], -1))

    def fc_wgrad_split(self, dh, x, dw_out, db_out, jobs, split_rows: int, jnorm, dh_lo=None, x_lo=None,
                       cpb: int = -1) -> int:
        if not self.native_conv:
            return super().fc_wgrad_split(dh, x, dw_out, db_out, jobs, split_rows, jnorm, dh_lo, x_lo, cpb)
        M = dh.shape[0]
        return C.dense_wgrad_split(self.lib, self.ws, dh, x.reshape(M, -1), max(1, -(-M // int(split_rows))),
                                   dw_out, db_out, jobs, dy_lo=dh_lo,
                                   x_lo=None if x_lo is None else x_lo.reshape(M, -1), cpb=cpb, jnorm=jnorm)

    def fc_head_wgrad(self, dh, x, dw_out, db_out, Hon, dhead, g_head, prio, norm=None, dh_lo=None, x_lo=None,
                      Hon_lo=None) -> int:
        # (the distributional head's wide weight gradient does not ride in the fused launch: the
        # head weight gradient + priority write-back launch, then the fc weight gradient)
        if self.native_conv and prio is not None and prio[0].use_hip and g_head["bv"].numel() == 1:
            rp, idx, gen, td = prio
            r = C.dense_wgrad_head_prio(self.lib, dh, x.reshape(x.shape[0], -1), dw_out, db_out, norm,
                                        self._head_wg(Hon, dhead, g_head, Hon_lo)[0], rp.tree_upd_args(idx, td, gen),
                                        dy_lo=dh_lo, x_lo=None if x_lo is None else x_lo.reshape(x.shape[0], -1))
            if r is not None:
                return r
        if self.native_conv and norm is not None and g_head["bv"].numel() > 1:
            # the wide head's blocks leave their own squared-norm partials, the fc partials follow
            nh = self.head_wgrad(Hon, dhead, g_head, prio=prio, Hon_lo=Hon_lo, norm=norm)
            return nh + self.fc_wgrad(dh, x, dw_out, db_out, norm=(norm[0], int(norm[1]) + nh), dh_lo=dh_lo, x_lo=x_lo)
        return super().fc_head_wgrad(dh, x, dw_out, db_out, Hon, dhead, g_head, prio, norm, dh_lo, x_lo, Hon_lo)

    def finalize_grads(self, jobs, norm_range=None, norm=None) -> int:
        """Returns the number of squared-norm partial slots written (``slot0`` + blocks)."""
        if not jobs and norm is None:
            return 0
        if norm is None:
            C.finalize_grads(self.lib, jobs)
            return 0
        return norm["slot0"] + C.finalize_grads(self.lib, jobs, norm_range, norm["part"], norm["slot0"],
                                                norm.get("total"))

    def conv_dgrad(self, dy, w, stride, x_src, dx_out, dy_lo=None, w_lo=None, dx_lo=None):
        if not self.native_conv:
            return super().conv_dgrad(dy, w, stride, x_src, dx_out, dy_lo, w_lo, dx_lo)
        if stride == 1:
            C.conv3_dgrad(self.lib, dy, w, x_src, dx_out, dy_lo=dy_lo, w_lo=w_lo, out_lo=dx_lo)
        else:
            key = (w.data_ptr(), _lib.ptr(w_lo))
            packed = getattr(self, "_c2d_packed", None) == key
            self._c2d_packed = None
            C.conv2_dgrad(self.lib, dy, w, x_src, dx_out, dy_lo=dy_lo, w_lo=w_lo, out_lo=dx_lo, ws=self.ws,
                          packed=packed)

    def conv_wgrad(self, dy, x, k, stride, dw_out, db_out, jobs=None, dy_lo=None, x_lo=None):
        if not self.native_conv:
            return super().conv_wgrad(dy, x, k, stride, dw_out, db_out, dy_lo=dy_lo, x_lo=x_lo)
        C.conv_wgrad(self.lib, self.ws, dy, x, k, stride, dw_out, db_out, jobs=jobs, dy_lo=dy_lo, x_lo=x_lo)

    def conv1_wgrad_ring(self, dy, ring, slots, frames_buf, scale, dw_out, db_out, jobs=None, dy_lo=None):
        if not self.native_conv:
            return super().conv1_wgrad_ring(dy, ring, slots, frames_buf, scale, dw_out, db_out, dy_lo=dy_lo)
        C.conv1_wgrad_ring(self.lib, self.ws, dy, ring, slots, scale, dw_out, db_out, jobs=jobs, dy_lo=dy_lo)

    def conv21_fused_ok(self, dy2, slots, dy2_lo=None, w2_lo=None) -> bool:
        # split mode, 4 frames, static image order (no work queue for this launch), and a batch
        # above the (image, class) data gradient's range, which spreads few images over the chip
        return bool(self.native_conv and SW.conv21_bwd_fused and SW.conv2_dgrad_img and dy2_lo is not None
                    and w2_lo is not None and slots.shape[1] == 4 and dy2.shape[0] > SW.conv2_dgrad_cls_max
                    and hasattr(self.lib, "apex_conv21_bwd_fused") and not self.ws.wq_on())

    def conv2_dgrad_conv1_wgrad(self, dy2, w2, y1, dy1, ring, slots, frames_buf, scale, dw_out, db_out, jobs=None,
                                dy2_lo=None, w2_lo=None, dy1_lo=None):
        # one kernel, dY1 in LDS only (csrc/conv21_bwd_fused.hip), where it applies; else the pair
        if self.conv21_fused_ok(dy2, slots, dy2_lo, w2_lo):
            packed = getattr(self, "_c2d_packed", None) == (w2.data_ptr(), _lib.ptr(w2_lo))
            self._c2d_packed = None
            C.conv2_dgrad_conv1_wgrad_fused(self.lib, self.ws, dy2, dy2_lo, w2, w2_lo, y1, ring, slots, scale,
                                            dw_out, db_out, jobs=jobs, packed=packed)
            return
        super().conv2_dgrad_conv1_wgrad(dy2, w2, y1, dy1, ring, slots, frames_buf, scale, dw_out, db_out, jobs=jobs,
                                        dy2_lo=dy2_lo, w2_lo=w2_lo, dy1_lo=dy1_lo)

    @staticmethod
    def _hp(P):
        h = _lib.HeadParams()
        h.wv, h.bv, h.wa, h.ba = (P["wv"].data_ptr(), P["bv"].data_ptr(), P["wa"].data_ptr(),
                                  P["ba"].data_ptr())
        return h

    def head(self, Hon, Htg, Pon, Ptg, act, rew, gam, isw, huber, kappa, grad_scale, td_abs, loss, dH,
             dhead, q_out=None, zero=None, lo=None, isn=None, rescale_eps=None):
        a = _lib.DdqnArgs()
        self._head_io(a.io, Hon, Htg, Pon, Ptg, act, rew, gam, isw, Pon["wa"].shape[0], Pon["wv"].numel(), grad_scale,
                      td_abs, loss, dH, dhead, q_out, zero, lo, isn, rescale_eps)
        a.huber, a.kappa = int(huber), float(kappa)
        hp, pk = a.hp, a.pk
        fp = getattr(self, "_fc_part", None)
        if fp is not None:
            # the deferred fc epilogue: h rows [0, B) (+ lo plane) are written by this launch
            self._fc_part = None
            assert fp["out"].data_ptr() == Hon.data_ptr() and fp["two_b"] == 2 * a.io.B
            hp.part, hp.zstride, hp.nz = fp["part"].data_ptr(), int(fp["zstride"]), int(fp["nz"])
            hp.bias_on, hp.bias_tg, hp.two_b = fp["b"].data_ptr(), fp["b2"].data_ptr(), int(fp["two_b"])
            hp.hon, hp.hon_lo = Hon.data_ptr(), _lib.ptr(None if lo is None else lo[0])
            if fp["c2d"] is not None:
                pk.w, pk.w_lo = fp["c2d"][0].data_ptr(), _lib.ptr(fp["c2d"][1])
                pk.out = C.c2d_wfrag_buffer(self.ws, Hon.device).data_ptr()
                self._c2d_packed = (fp["c2d"][0].data_ptr(), _lib.ptr(fp["c2d"][1]))
        _lib.check(self.lib.apex_ddqn_head(a, _lib.stream_ptr()), "ddqn_head")

    def value_rescale_probe(self, y, R, Gamma, eps, out) -> None:
        """csrc/ddqn_head.hip ``value_rescale_probe_kernel``: ``out[i] = T(R[i], Gamma[i], y[i], eps)`` of
        csrc/value_rescale.h, element-wise on fp32 vectors (the unit test of the device function)."""
        n = out.numel()
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n for t in (y, R, Gamma, out))
        _lib.check(self.lib.apex_value_rescale_probe(y.data_ptr(), R.data_ptr(), Gamma.data_ptr(),
                                                     _lib.rescale_eps_arg(eps), out.data_ptr(), n, _lib.stream_ptr()),
                   "value_rescale_probe")

    def _head_io(self, io, Hon, Htg, Pon, Ptg, act, rew, gam, isw, A, hidden, grad_scale, td_abs, loss, dH, dhead,
                 q_out, zero, lo, isn, rescale_eps=None) -> None:
        """Fill ``io``, the block every struct-argument head takes (``_lib.HeadIO``); ``B`` is ``act``'s."""
        io.Hon, io.Htg, io.Pon, io.Ptg = Hon.data_ptr(), Htg.data_ptr(), self._hp(Pon), self._hp(Ptg)
        io.act, io.rew, io.gam, io.isw = act.data_ptr(), rew.data_ptr(), gam.data_ptr(), _lib.ptr(isw)
        io.B, io.A, io.hidden, io.grad_scale = act.shape[0], int(A), int(hidden), float(grad_scale)
        io.td_abs, io.loss, io.q_out = td_abs.data_ptr(), loss.data_ptr(), _lib.ptr(q_out)
        io.dH, io.dhead = dH.data_ptr(), dhead.data_ptr()
        io.zero_ptr, io.zero_n = _lib.ptr(zero), 0 if zero is None else zero.numel()
        io.lo = _lib.head_lo(*(lo if lo is not None else (None, None, None)))
        io.isn = _lib.is_norm(isn)
        io.rescale_eps = _lib.rescale_eps_arg(rescale_eps)

    def mdqn_head(self, Hon, Htg, Pon, Ptg, act, rew, gam, isw, huber, kappa, alpha, tau, clip, grad_scale, td_abs,
                  loss, dH, dhead, q_out=None, aux=None, zero=None, lo=None, isn=None):
        """csrc/mdqn_head.hip ``mdqn_head_kernel`` (reads h: with the weight set switched at row B the fc
        forward never defers its epilogue)."""
        assert getattr(self, "_fc_part", None) is None, "the Munchausen head reads h: fc epilogue deferred"
        a = _lib.MdqnArgs()
        B, A = act.shape[0], Pon["wa"].shape[0]
        self._head_io(a.io, Hon, Htg, Pon, Ptg, act, rew, gam, isw, A, Pon["wv"].numel(), grad_scale, td_abs, loss, dH,
                      dhead, q_out, zero, lo, isn)
        a.huber, a.kappa, a.alpha, a.tau, a.clip = int(huber), float(kappa), float(alpha), float(tau), float(clip)
        a.aux = _lib.ptr(aux)
        assert Hon.shape[0] == B and Htg.shape[0] == 2 * B and Hon.is_contiguous() and Htg.is_contiguous()
        assert dhead.shape == (B, A + 1) and dhead.is_contiguous() and dH.is_contiguous()
        assert aux is None or (aux.shape == (B, 2) and aux.dtype == torch.float32 and aux.is_contiguous())
        assert q_out is None or (q_out.shape == (B, A) and q_out.is_contiguous())
        _lib.check(self.lib.apex_mdqn_head(a, _lib.stream_ptr()), "mdqn_head")

    def _dist_head_launch(self, a, symbol, Hon, Htg, Pon, Ptg, act, rew, gam, isw, num_atoms, grad_scale, td_abs, loss,
                          dH, dhead, q_out, zero, lo, isn, rescale_eps) -> None:
        """Launch ``apex_<symbol>`` with the argument struct ``a``, whose scalar fields but ``N`` the caller has
        set (the three heads of csrc/dist_head.h's frame; they read h: the fc epilogue is not deferred)."""
        assert getattr(self, "_fc_part", None) is None, "the distributional head reads h: fc epilogue deferred"
        a.N = N = int(num_atoms)
        B, A = act.shape[0], Pon["wa"].shape[0] // N
        self._head_io(a.io, Hon, Htg, Pon, Ptg, act, rew, gam, isw, A, Pon["wv"].shape[-1], grad_scale, td_abs, loss,
                      dH, dhead, q_out, zero, lo, isn, rescale_eps)
        assert dhead.shape == (B, (A + 1) * N) and dhead.is_contiguous()
        _lib.check(getattr(self.lib, "apex_" + symbol)(a, _lib.stream_ptr()), symbol)

    def c51_head(self, Hon, Htg, Pon, Ptg, act, rew, gam, isw, num_atoms, v_min, v_max, grad_scale, td_abs, loss,
                 dH, dhead, q_out=None, zero=None, lo=None, isn=None, rescale_eps=None):
        """csrc/c51_head.hip ``c51_head_kernel``."""
        a = _lib.C51Args()
        a.vmin, a.vmax = float(v_min), float(v_max)
        self._dist_head_launch(a, "c51_head", Hon, Htg, Pon, Ptg, act, rew, gam, isw, num_atoms, grad_scale, td_abs,
                               loss, dH, dhead, q_out, zero, lo, isn, rescale_eps)

    def hlg_head(self, Hon, Htg, Pon, Ptg, act, rew, gam, isw, num_atoms, v_min, v_max, sigma_ratio, grad_scale,
                 td_abs, loss, dH, dhead, q_out=None, zero=None, lo=None, isn=None, rescale_eps=None):
        """csrc/c51_head.hip ``hlg_head_kernel``."""
        a = _lib.HlgArgs()
        a.vmin, a.vmax, a.sigma_ratio = float(v_min), float(v_max), float(sigma_ratio)
        self._dist_head_launch(a, "hlg_head", Hon, Htg, Pon, Ptg, act, rew, gam, isw, num_atoms, grad_scale, td_abs,
                               loss, dH, dhead, q_out, zero, lo, isn, rescale_eps)

    def _actor_io(self, io, H, P, eps, ctr, seed, q_out, a_out, H_lo) -> None:
        """Fill ``io``, the block every actor head takes (``_lib.ActorIO``); ``E`` and ``A`` are ``q_out``'s."""
        io.H, io.H_lo, io.P = H.data_ptr(), _lib.ptr(H_lo), self._hp(P)
        (io.E, io.A), io.hidden = q_out.shape, P["wv"].shape[-1]
        io.eps, io.seed, io.ctr = eps.data_ptr(), int(seed), ctr.data_ptr()
        io.q_out, io.a_out = q_out.data_ptr(), a_out.data_ptr()

    def c51_actor_head(self, H, P, eps, ctr, seed, num_atoms, v_min, v_max, q_out, a_out, H_lo=None):
        a = _lib.C51ActorArgs()
        self._actor_io(a.io, H, P, eps, ctr, seed, q_out, a_out, H_lo)
        a.N, a.vmin, a.vmax = int(num_atoms), float(v_min), float(v_max)
        _lib.check(self.lib.apex_c51_actor_head(a, _lib.stream_ptr()), "c51_actor_head")

    def qr_head(self, Hon, Htg, Pon, Ptg, act, rew, gam, isw, num_atoms, kappa, grad_scale, td_abs, loss,
                dH, dhead, q_out=None, zero=None, lo=None, isn=None, rescale_eps=None):
        """csrc/qr_head.hip ``qr_head_kernel``."""
        a = _lib.QRArgs()
        a.kappa = float(kappa)
        self._dist_head_launch(a, "qr_head", Hon, Htg, Pon, Ptg, act, rew, gam, isw, num_atoms, grad_scale, td_abs,
                               loss, dH, dhead, q_out, zero, lo, isn, rescale_eps)

    def qr_actor_head(self, H, P, eps, ctr, seed, num_atoms, q_out, a_out, H_lo=None):
        a = _lib.QRActorArgs()
        self._actor_io(a.io, H, P, eps, ctr, seed, q_out, a_out, H_lo)
        a.N = int(num_atoms)
        _lib.check(self.lib.apex_qr_actor_head(a, _lib.stream_ptr()), "qr_actor_head")

    @staticmethod
    def _embed(E):
        e = _lib.IqnEmbed()
        assert E["wtau"].is_contiguous() and E["wtau"].shape[-1] == 64 and E["btau"].numel() == E["wtau"].shape[0]
        e.w, e.b = E["wtau"].data_ptr(), E["btau"].data_ptr()
        return e

    def iqn_workspace(self, B: int, N: int, device, dtype=torch.float32) -> Dict[str, torch.Tensor]:
        """The torch backend's buffers plus ``wpart``: the split partials of G[wtau | btau] that the weight
        gradient leaves for its reduce launch (allocated here, never inside a capture)."""
        ws = super().iqn_workspace(B, N, device, dtype)
        ws["wpart"] = torch.zeros(self.lib.apex_iqn_wgrad_part_floats(), dtype=torch.float32, device=device)
        return ws

    def iqn_head(self, Hon, Htg, Pon, Ptg, Eon, Etg, act, rew, gam, isw, num_samples, kappa, grad_scale, seed_q, ctr,
                 base, td_abs, loss, dH, dhead, ws, q_out=None, tau_out=None, zero=None, lo=None, isn=None,
                 max_blocks=None, rescale_eps=None):
        """csrc/iqn_head.hip ``iqn_head_kernel`` (reads h: the fc epilogue is not deferred).  ``max_blocks``
        caps the persistent grid (default: the CU count)."""
        assert getattr(self, "_fc_part", None) is None, "the distributional head reads h: fc epilogue deferred"
        N = int(num_samples)
        a = _lib.IqnArgs()
        B, A, hidden = act.shape[0], Pon["wa"].shape[0], Pon["wv"].shape[-1]
        self._head_io(a.io, Hon, Htg, Pon, Ptg, act, rew, gam, isw, A, hidden, grad_scale, td_abs, loss, dH, dhead,
                      q_out, zero, lo, isn, rescale_eps)
        a.N, a.kappa, a.seed_q = N, float(kappa), int(seed_q)
        assert ctr.dtype == torch.int64 and (base is None or base.dtype == torch.int64)
        a.ctr, a.base = ctr.data_ptr(), _lib.ptr(base)
        a.Eon, a.Etg, a.tau_out = self._embed(Eon), self._embed(Etg), _lib.ptr(tau_out)
        a.dpre, a.cosT, a.xg, a.gsum = (ws["dpre"].data_ptr(), ws["cos"].data_ptr(), ws["xg"].data_ptr(),
                                        ws["gsum"].data_ptr())
        a.max_blocks = 0 if max_blocks is None else int(max_blocks)
        assert Pon["wv"].numel() == hidden and Ptg["wv"].numel() == hidden and Eon["wtau"].shape[0] == 2 * hidden
        assert Hon.shape[0] >= 2 * B and Htg.shape[0] >= B and Hon.is_contiguous() and Htg.is_contiguous()
        assert dhead.shape == (B, (A + 1) * N) and dhead.is_contiguous() and dhead.dtype == torch.float32
        assert dH.shape == (B, 2 * hidden) and dH.is_contiguous()
        assert ws["dpre"].shape == (B, N, 2 * hidden) and ws["cos"].shape == (B, N, 64)
        assert ws["xg"].shape == (B, 2 * hidden) and ws["gsum"].shape == (B,)
        assert all(ws[k].dtype == torch.float32 and ws[k].is_contiguous() for k in ("dpre", "cos", "xg", "gsum"))
        assert tau_out is None or (tau_out.shape == (B, 3, N) and tau_out.is_contiguous()
                                   and tau_out.dtype == torch.float32)
        assert q_out is None or (q_out.shape == (B, A) and q_out.is_contiguous())
        _lib.check(self.lib.apex_iqn_head(a, _lib.stream_ptr()), "iqn_head")

    def iqn_wgrad(self, act, ws, g, prio=None) -> None:
        """csrc/sumtree.hip ``iqn_wgrad_prio_kernel`` + ``iqn_wgrad_reduce_kernel`` (csrc/iqn_wgrad.h): G[wv, bv, wa, ba, wtau, btau];
        ``prio = (replay, idx, gen, td_abs)``: block 0 of the same launch writes the priorities back."""
        h = _lib.IqnWgArgs()
        B, N = ws["dpre"].shape[0], ws["dpre"].shape[1]
        A, HS = g["wa"].shape
        h.dpre, h.cosT, h.xg, h.gsum = (ws["dpre"].data_ptr(), ws["cos"].data_ptr(), ws["xg"].data_ptr(),
                                        ws["gsum"].data_ptr())
        h.act, h.B, h.A, h.N = act.data_ptr(), B, A, N
        assert act.shape == (B,) and act.dtype == torch.int32 and HS == 512
        assert g["wv"].numel() == HS and g["bv"].numel() == 1 and g["ba"].numel() == A
        assert g["wtau"].shape == (2 * HS, 64) and g["btau"].numel() == 2 * HS
        assert all(g[k].is_contiguous() and g[k].dtype == torch.float32 for k in ("wv", "bv", "wa", "ba", "wtau", "btau"))
        h.gwv, h.gbv, h.gwa, h.gba = g["wv"].data_ptr(), g["bv"].data_ptr(), g["wa"].data_ptr(), g["ba"].data_ptr()
        h.gwtau, h.gbtau = g["wtau"].data_ptr(), g["btau"].data_ptr()
        assert ws["wpart"].numel() == self.lib.apex_iqn_wgrad_part_floats() and ws["wpart"].dtype == torch.float32
        h.part = ws["wpart"].data_ptr()
        if prio is not None and prio[0].use_hip and B <= 1024:
            rp, idx, gen, td = prio
            _lib.check(self.lib.apex_iqn_wgrad_prio(h, rp.tree_upd_args(idx, td, gen), _lib.stream_ptr()),
                       "iqn_wgrad_prio")
            return
        if prio is not None:
            prio[0].update_priorities(prio[1], prio[3], prio[2])
        _lib.check(self.lib.apex_iqn_wgrad(h, _lib.stream_ptr()), "iqn_wgrad")

    def iqn_actor_head(self, H, P, E, eps, ctr, seed, seed_q, tau_ctr, stream, num_samples, midpoint, q_out, a_out,
                       H_lo=None, tau_out=None):
        """csrc/iqn_head.hip ``iqn_actor_head_kernel``."""
        a = _lib.IqnActorArgs()
        n_e, A = q_out.shape
        self._actor_io(a.io, H, P, eps, ctr, seed, q_out, a_out, H_lo)
        a.Em, a.K, a.midpoint = self._embed(E), int(num_samples), int(bool(midpoint))
        a.seed_q, a.tau_ctr, a.stream, a.tau_out = int(seed_q), _lib.ptr(tau_ctr), int(stream), _lib.ptr(tau_out)
        assert H.shape[0] >= n_e and H.shape[1] == 2 * a.io.hidden and H.is_contiguous() and P["wa"].shape[0] == A
        assert eps.numel() >= n_e and a_out.numel() >= n_e and q_out.is_contiguous()
        assert tau_ctr is None or tau_ctr.dtype == torch.int64
        assert tau_out is None or (tau_out.shape == (n_e, a.K) and tau_out.is_contiguous())
        _lib.check(self.lib.apex_iqn_actor_head(a, _lib.stream_ptr()), "iqn_actor_head")

    @staticmethod
    def _head_wg(Hon, dhead, g, Hon_lo=None, norm=None):
        """``HeadWgArgs`` of a head weight gradient and the norm slots its blocks write (``norm =
        (partials, slot0)``, the distributional head only)."""
        B, J = dhead.shape
        nv = g["bv"].numel()          # value rows: 1, or the distributional head's atoms
        h = _lib.HeadWgArgs(Hon=Hon.data_ptr(), Hon_lo=_lib.ptr(Hon_lo), dhead=dhead.data_ptr(), B=B, A=J - nv, NV=nv,
                            HS=g["wv"].shape[-1], gwv=g["wv"].data_ptr(), gbv=g["bv"].data_ptr(),
                            gwa=g["wa"].data_ptr(), gba=g["ba"].data_ptr())
        nslots = 0
        if norm is not None:
            assert nv >= 2
            nslots = (-(-nv // 8) + -(-(J - nv) // 8)) * (h.HS // 64)       # csrc/head_common.h HWG_JT
            h.norm_part = norm[0].data_ptr() + 8 * int(norm[1])
            assert int(norm[1]) + nslots <= norm[0].numel() and norm[0].dtype == torch.float64
        return h, nslots

    def head_wgrad(self, Hon, dhead, g, prio=None, Hon_lo=None, pack=None, norm=None) -> int:
        """``norm = (partials, slot0)`` (the distributional head only): every block also leaves
        the squared norm of what it stores; returns the slots written."""
        h, nslots = self._head_wg(Hon, dhead, g, Hon_lo, norm)
        if prio is not None and prio[0].use_hip and h.B <= 1024:
            rp, idx, gen, td = prio
            pk = self._pack_args(*pack) if pack is not None else (None, None, None, 0, 0, None, 0)
            _lib.check(self.lib.apex_head_wgrad_prio(h, rp.tree_upd_args(idx, td, gen), *pk, _lib.stream_ptr()),
                       "head_wgrad_prio")
            return nslots
        if pack is not None:
            self.pack_rows(*pack)
        if prio is not None:
            prio[0].update_priorities(prio[1], prio[3], prio[2])
        _lib.check(self.lib.apex_head_wgrad(h, _lib.stream_ptr()), "head_wgrad")
        return nslots

    def actor_head(self, H, P, eps, ctr, seed, q_out, a_out, H_lo=None):
        a = _lib.ActorIO()
        self._actor_io(a, H, P, eps, ctr, seed, q_out, a_out, H_lo)
        _lib.check(self.lib.apex_actor_head(a, _lib.stream_ptr()), "actor_head")

    @staticmethod
    def _opt_sched(opt) -> "_lib.OptSched":
        """``OptSched`` of an ``OptSpec`` (all-zero for None: RMSprop, lr by value)."""
        os_ = _lib.OptSched()
        if opt is not None:
            os_.ctr, os_.base, os_.adam = _lib.ptr(opt.ctr), _lib.ptr(opt.base), int(opt.adam)
            os_.warmup, os_.decay = int(opt.warmup), int(opt.decay)
            os_.lr0, os_.lr_end = float(opt.lr), float(opt.lr if opt.lr_end is None else opt.lr_end)
            os_.beta1, os_.beta2 = float(opt.beta1), float(opt.beta2)
            if opt.t0 is not None:     # (only with Runtime.reset_interval: else the arguments of before)
                assert opt.adam and opt.t0.dtype == torch.int64
                os_.t0 = opt.t0.data_ptr()
        return os_

    def _opt_args(self, p32, g32, v, m, pbf, lr, alpha, eps, clip, centered, norm_out, pb_lo, wnorm, frag_out,
                  norm_prefix, opt, target) -> "_lib.RmspropArgs":
        """``RmspropArgs`` of an optimizer launch, but for the clip norm's partials (``partials``, ``npart``)."""
        n = p32.numel()
        if opt is not None and opt.adam:
            eps = opt.adam_eps        # (RmspropArgs.eps carries Adam's epsilon)
        a = _lib.RmspropArgs(p=p32.data_ptr(), g=g32.data_ptr(), v=v.data_ptr(), m=m.data_ptr(), pb=pbf.data_ptr(),
                             pb_lo=_lib.ptr(pb_lo), n=n, lr=float(lr), alpha=float(alpha), eps=float(eps),
                             clip=float(clip), centered=int(centered), norm_out=norm_out.data_ptr(),
                             os=self._opt_sched(opt), gpre=_lib.ptr(norm_prefix),
                             npre=0 if norm_prefix is None else norm_prefix.numel())
        if wnorm is not None:
            a.wnorm, a.wn, a.wstride = wnorm[0].data_ptr(), int(wnorm[1]), int(wnorm[2])
        if frag_out is not None:
            a.fo = frag_out
        if target is not None:
            t32, tbf, tbf_lo, rho, tfo = target
            assert t32.dtype == torch.float32 and t32.numel() == n and tbf.numel() == n and tbf.dtype == pbf.dtype \
                and (tbf_lo is None) == (pb_lo is None) and (tbf_lo is None or tbf_lo.numel() == n)
            a.tg = _lib.OptTarget(t32.data_ptr(), tbf.data_ptr(), _lib.ptr(tbf_lo), float(rho),
                                  _lib.CfFragOut() if tfo is None else tfo)
        return a

    def optimizer(self, p32, g32, v, m, pbf, lr, alpha, eps, clip, centered, partials, norm_out, norm_total=None,
                  sample=None, pb_lo=None, wnorm=None, frag_out=None, segs=None, norm_prefix=None, opt=None,
                  target=None) -> bool:
        """``frag_out`` (ops/conv.py conv12_frag_out): the launch also stores the updated
        w1 / w2 in the fused forward's fragment order.  Returns whether it did (the fused
        optimizer + sample launch only).  ``segs``: the ranges to update (the sharded DP
        update: one launch, csrc/sumtree.hip ``RmsSegs``).  ``target``: the soft target net, averaged in the
        same launch (csrc/rmsprop_common.h ``OptTarget``)."""
        # the next batch's draw rides in the optimizer launch (csrc/sumtree.hip: rmsprop_sample_kernel)
        fused = sample is not None and sample[0].use_hip
        if target is not None and segs is not None:
            raise ValueError("the soft target is averaged over the whole parameter vector, not in a sharded update")
        if target is not None and target[4] is not None and frag_out is None:
            raise ValueError("the target's fragment stores ride beside the online ones (frag_out)")
        if segs is not None and norm_total is None:
            raise ValueError("a sharded update needs the clip norm's partials (norm_total)")
        for name, arg in (("segs", segs), ("frag_out", frag_out), ("norm_prefix", norm_prefix)):
            if arg is not None and not fused:
                raise ValueError(f"{name} needs the fused optimizer + sample launch (a HIP replay)")
        if sample is not None and not fused:
            self.optimizer(p32, g32, v, m, pbf, lr, alpha, eps, clip, centered, partials, norm_out, norm_total,
                           pb_lo=pb_lo, wnorm=wnorm, opt=opt, target=target)
            rp, B, out, nxt2, obs2 = _sample5(sample)
            rp.sample(B, out=out, nxt2=nxt2, **({} if obs2 is None else {"obs2": obs2}))
            return
        a = self._opt_args(p32, g32, v, m, pbf, lr, alpha, eps, clip, centered, norm_out, pb_lo, wnorm, frag_out,
                           norm_prefix, opt, target)
        if norm_total is None:                # the optimizer's own squared-norm pass
            norm_total = (partials, self.grad_sqnorm_partials(g32, partials))
        # (producer partials, count), summed in the launch; or the total
        part, a.npart = norm_total if isinstance(norm_total, tuple) else (norm_total, 1)
        a.partials = part.data_ptr()
        if not fused:
            _lib.check(self.lib.apex_opt_step(a, _lib.stream_ptr()), "opt_step")
            return
        rp, B, out, nxt2, obs2 = _sample5(sample)
        sg = None if segs is None else _lib.RmsSegs(nseg=len(segs))
        for k, (o, ln) in enumerate(segs or ()):      # (at most three: the launcher checks nseg)
            sg.off[k], sg.len[k] = int(o), int(ln)
        _lib.check(self.lib.apex_opt_sample(a, rp.sample_launch_args(B, out, nxt2, obs2),
                                            None if sg is None else ctypes.byref(sg), _lib.stream_ptr()), "opt_sample")
        return frag_out is not None

    def _pack_args(self, dst: torch.Tensor, segs):
        """(src*, ld*, cols*, nseg, rows, dst, dst ld) of a row pack (csrc/pack_rows.h); the
        ctypes arrays stay referenced by this backend until the next call."""
        assert dst.dtype in (torch.bfloat16, torch.float16) and len(segs) <= 4
        n = len(segs)
        src = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in segs])
        ld = (ctypes.c_int64 * 4)(*[t.stride(0) for t in segs])
        cols = (ctypes.c_int * 4)(*[t.reshape(t.shape[0], -1).shape[1] for t in segs])
        for t in segs:
            assert t.dtype == dst.dtype and t.reshape(t.shape[0], -1).stride(1) == 1 and t.shape[0] == segs[0].shape[0]
        self._pack_keep = (src, ld, cols)
        return (ctypes.addressof(src), ctypes.addressof(ld), ctypes.addressof(cols), n, int(segs[0].shape[0]),
                dst.data_ptr(), int(dst.stride(0)))

    def pack_rows(self, dst: torch.Tensor, segs) -> None:
        if dst.dtype not in (torch.bfloat16, torch.float16) or len(segs) > 4:
            return super().pack_rows(dst, segs)
        _lib.check(self.lib.apex_pack_rows(*self._pack_args(dst, segs), _lib.stream_ptr()), "pack_rows")

    def grad_sqnorm_partials(self, g32, partials) -> int:
        """Squared-norm partials of the whole gradient (the optimizer's own pass);
        returns the partial count."""
        assert partials.numel() >= _lib.SQNORM_PARTIALS
        _lib.check(self.lib.apex_grad_sqnorm_partials(g32.data_ptr(), g32.numel(), partials.data_ptr(),
                                                      _lib.stream_ptr()), "sqnorm")
        return _lib.SQNORM_PARTIALS

    def sqnorm_ranges(self, ranges, partials: torch.Tensor, nblk: int) -> int:
        (a, b) = (list(ranges) + [None])[:2]
        _lib.check(self.lib.apex_sqnorm_ranges(a.data_ptr(), a.numel(), _lib.ptr(b), 0 if b is None else b.numel(),
                                               partials.data_ptr(), int(nblk), _lib.stream_ptr()), "sqnorm_ranges")
        return int(nblk)

    @staticmethod
    def _noisy_offsets(plan, mu, sg) -> None:
        from ..learner import noisy as NZ
        for k, name in enumerate(NZ.MU):
            mu[k], sg[k] = int(plan.offsets[name]), int(plan.offsets[NZ.SIGMA[name]])

    def noisy_compose(self, plan, nets, xi, fc32=None, xi_in=None) -> None:
        """csrc/noisy.hip ``noisy_compose_kernel``: all nets in one launch; the draw index is
        read on the device."""
        if xi_in is not None:
            return super().noisy_compose(plan, nets, xi, fc32, xi_in)
        a = _lib.NoisyArgs()
        a.nnets, a.A, a.N, a.stream0 = len(nets), int(plan.A), int(plan.N), int(plan.stream0)
        assert 1 <= a.nnets <= 2 and xi.dtype == torch.float32 and xi.shape[0] >= a.nnets and xi.shape[1] >= plan.K \
            and xi.stride(1) == 1 and xi.stride(0) % 4 == 0
        self._noisy_offsets(plan, a.mu, a.sg)
        a.seed, a.ctr, a.base, a.every = int(plan.seed), plan.ctr.data_ptr(), _lib.ptr(plan.base), int(plan.every)
        assert plan.ctr.dtype == torch.int64 and (plan.base is None or plan.base.dtype == torch.int64)
        a.n_p = min(int(p.numel()) for p, _, _, _ in nets)
        a.n_e = min(min(int(e.numel()), int(h.numel()), int(h.numel() if l is None else l.numel()))
                    for _, e, h, l in nets)
        for i, (p, e32, ehi, elo) in enumerate(nets):
            assert p.dtype == torch.float32 and e32.dtype == torch.float32 and ehi.dtype == torch.bfloat16 \
                and (elo is None or elo.dtype == torch.bfloat16)
            n = a.net[i]
            n.p, n.e32, n.ehi, n.elo, n.xi = p.data_ptr(), e32.data_ptr(), ehi.data_ptr(), _lib.ptr(elo), \
                xi[i].data_ptr()
            f = None if fc32 is None else fc32[i]
            assert f is None or (f.dtype == torch.float32 and f.is_contiguous() and f.numel() == 1024 * 3136)
            n.fc32 = _lib.ptr(f)
        _lib.check(self.lib.apex_noisy_compose(a, _lib.stream_ptr()), "noisy_compose")

    def noisy_sigma_grad(self, plan, g32, xi) -> None:
        """csrc/noisy.hip ``noisy_sigma_grad_kernel``."""
        a = _lib.NoisyGradArgs()
        assert g32.dtype == torch.float32 and xi.dtype == torch.float32 and xi.numel() >= plan.K and xi.is_contiguous()
        a.g, a.xi, a.A, a.N, a.n_g = g32.data_ptr(), xi.data_ptr(), int(plan.A), int(plan.N), int(g32.numel())
        self._noisy_offsets(plan, a.mu, a.sg)
        _lib.check(self.lib.apex_noisy_sigma_grad(a, _lib.stream_ptr()), "noisy_sigma_grad")

    def augment_args(self, ring, slots, pad, seed, ctr, base, out, off_out) -> "_lib.AugArgs":
        """The argument block of ``apex_augment_shift`` (tests pass altered copies to the launcher)."""
        rows, C = self._augment_check(ring, slots, pad, ctr, base, out, off_out)
        a = _lib.AugArgs()
        a.ring, a.F, a.slots, a.rows, a.C, a.pad = ring.data_ptr(), int(ring.shape[0]), slots.data_ptr(), rows, C, int(pad)
        a.seed, a.ctr, a.base = int(seed), ctr.data_ptr(), _lib.ptr(base)
        a.out, a.n_out, a.off_out = out.data_ptr(), int(out.numel()), off_out.data_ptr()
        return a

    def augment_shift(self, ring, slots, pad, seed, ctr, base, out, off_out) -> None:
        """csrc/augment.hip ``augment_shift_kernel``: one launch; the update index is read on the device."""
        a = self.augment_args(ring, slots, pad, seed, ctr, base, out, off_out)
        _lib.check(self.lib.apex_augment_shift(a, _lib.stream_ptr()), "augment_shift")

    def reset_args(self, table, seed, r, p32, t32, v, m, pb, tb) -> "_lib.ResetArgs":
        """The argument block of ``apex_reset_perturb`` (tests pass altered copies to the launcher)."""
        n = self._reset_check(table, p32, t32, v, m, pb, tb)
        assert self.lib.apex_reset_args_size() == ctypes.sizeof(_lib.ResetArgs)
        a = _lib.ResetArgs(p=p32.data_ptr(), t=t32.data_ptr(), v=v.data_ptr(), m=m.data_ptr(), pb=pb[0].data_ptr(),
                           tb=tb[0].data_ptr(), pb_lo=_lib.ptr(pb[1]), tb_lo=_lib.ptr(tb[1]), n=n,
                           seed=int(seed), r=int(r), nrows=len(table))
        for k, row in enumerate(table):
            a.rows[k] = _lib.ResetRow(*row)
        return a

    def reset_perturb(self, table, seed, r, p32, t32, v, m, pb, tb) -> None:
        """csrc/reset.hip ``reset_perturb_kernel``: one launch over the flat vector."""
        a = self.reset_args(table, seed, r, p32, t32, v, m, pb, tb)
        _lib.check(self.lib.apex_reset_perturb(a, _lib.stream_ptr()), "reset_perturb")

    def cast_bf16(self, x32, hi, lo=None) -> None:
        """hi = bf16(x32) (and lo = bf16(x32 - hi)) with one kernel."""
        _lib.check(self.lib.apex_cast_bf16(x32.data_ptr(), hi.data_ptr(), x32.numel(), _lib.ptr(lo),
                                           _lib.stream_ptr()), "cast_bf16")
