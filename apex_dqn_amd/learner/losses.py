"""Double-DQN n-step loss (PyTorch oracle).

Reference ``learner.py:29-52`` computes ``G = R + Gamma * Q_double(S_tpn)[argmax Q(S_tpn)]``
and ``0.5*delta^2`` with no terminal mask, no IS weights and a broken
priority dict.  This module is the intended version:
terminal masking through Gamma=0 (set by the n-step builder), Huber (or
0.5*delta^2 for parity) weighted by IS weights, one |delta| per sample.
The fused HIP head kernel (``ops/kernels.py::ddqn_head``) is tested against
this function.
"""
from __future__ import annotations

from typing import Tuple

import torch

from .rescale import rescale_target


def huber(delta: torch.Tensor, kappa: float = 1.0) -> torch.Tensor:
    a = delta.abs()
    return torch.where(a <= kappa, 0.5 * delta * delta, kappa * (a - 0.5 * kappa))


def ddqn_targets(q_online_next: torch.Tensor, q_target_next: torch.Tensor,
                 R: torch.Tensor, Gamma: torch.Tensor, rescale_eps: float = None) -> torch.Tensor:
    """``rescale_eps`` (``Runtime.value_rescale``): T = h(R + Gamma h^-1(q_target[a*])), learner/rescale.py."""
    a_star = q_online_next.argmax(dim=1, keepdim=True)
    if rescale_eps is not None:
        return rescale_target(R, Gamma, q_target_next.gather(1, a_star).squeeze(1), float(rescale_eps))
    return R + Gamma * q_target_next.gather(1, a_star).squeeze(1)


def c51_project(p_next: torch.Tensor, R: torch.Tensor, Gamma: torch.Tensor, v_min: float,
                v_max: float, rescale_eps: float = None) -> torch.Tensor:
    """Categorical projection of the n-step target ``R + Gamma z`` onto the support
    z_i = v_min + i delta (N atoms): ``m_i = sum_j p'_j max(0, 1 - |b_j - i|)`` with
    ``b_j = (clamp(R + Gamma z_j, v_min, v_max) - v_min) / delta`` -- the usual floor / ceil
    split written as a gather (deterministic, continuous in b, no scatter), summed in
    increasing j.  Gamma = 0 (terminal) needs no special case; sum_i m_i = 1.  Computes in
    ``p_next``'s dtype (fp64 inputs: the tests' reference).  p_next [B, N] -> m [B, N].
    ``rescale_eps`` (``Runtime.value_rescale``): the support lives in transformed space and the atoms move
    to ``clamp(h(R + Gamma h^-1(z_j)), v_min, v_max)`` (learner/rescale.py)."""
    N = p_next.shape[-1]
    dt = p_next.dtype
    delta = (float(v_max) - float(v_min)) / (N - 1)
    idx = torch.arange(N, dtype=dt, device=p_next.device)
    z = float(v_min) + idx * delta
    if rescale_eps is not None:
        tz = rescale_target(R.to(dt)[:, None], Gamma.to(dt)[:, None], z[None, :], float(rescale_eps))
    else:
        tz = R.to(dt)[:, None] + Gamma.to(dt)[:, None] * z[None, :]
    tz = tz.clamp(float(v_min), float(v_max))
    b = (tz - float(v_min)) / delta
    m = torch.zeros_like(p_next)
    for j in range(N):        # fixed order: the kernels' sum
        m = m + p_next[:, j:j + 1] * (1.0 - (b[:, j:j + 1] - idx[None, :]).abs()).clamp_min(0.0)
    return m


def c51_loss(logp_t: torch.Tensor, q_online_next: torch.Tensor, p_target_next: torch.Tensor,
             A: torch.Tensor, R: torch.Tensor, Gamma: torch.Tensor, v_min: float, v_max: float,
             weights: torch.Tensor = None, rescale_eps: float = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Distributional double-DQN loss.  ``logp_t`` [B, A, N]: log p(S_t) of the online net;
    ``q_online_next`` [B, A]: its expected q at S_{t+n} (picks a*, first maximum);
    ``p_target_next`` [B, A, N]: the target net's probabilities at S_{t+n}.  Returns (mean
    over the batch of -w sum_i m_i log p(S_t)[a, i], |sum_i m_i z_i - q(S_t)[a]| per sample):
    the priority is the absolute TD error of the expectations, on the scale of the actors'
    initial priorities, not the KL."""
    B, _, N = logp_t.shape
    dt = logp_t.dtype
    ar = torch.arange(B, device=logp_t.device)
    with torch.no_grad():
        a_star = q_online_next.argmax(dim=1)
        m = c51_project(p_target_next[ar, a_star].to(dt), R, Gamma, v_min, v_max, rescale_eps)
        delta = (float(v_max) - float(v_min)) / (N - 1)
        z = float(v_min) + torch.arange(N, dtype=dt, device=logp_t.device) * delta
    lp = logp_t[ar, A.long().view(-1)]
    per = -(m * lp).sum(-1)
    if weights is not None:
        per = per * weights.to(dt)
    with torch.no_grad():
        td = ((m * z).sum(-1) - (lp.exp() * z).sum(-1)).abs()
    return per.mean(), td


def _f32(x: float) -> float:
    return float(torch.tensor(float(x), dtype=torch.float32))


def hl_gauss_target(y0: torch.Tensor, v_min: float, v_max: float, num_atoms: int,
                    sigma_ratio: float = 0.75) -> torch.Tensor:
    """The Gaussian histogram (HL-Gauss) target row of the scalar target ``y0`` [B] on the categorical head's
    support (Imani & White 2018; Farebrother et al. 2024), ``Runtime.dist_head = "hl_gauss"``.  Bins are centred
    on the C51 atoms z_i = v_min + i delta, delta = (v_max - v_min) / (N - 1)::

        sigma = sigma_ratio delta
        e_i   = v_min + (i - 1/2) delta,  i = 0..N          (N + 1 edges; bin i = [e_i, e_i+1], centre z_i)
        y     = clamp(y0, v_min, v_max)
        E_i   = erf((e_i - y) / (sigma sqrt 2))
        m_i   = (E_i+1 - E_i) / (E_N - E_0)                 (Gaussian mass of bin i, renormalised to the covered
                                                             range: sum_i m_i = 1)

    Evaluated in fp64 on the fp32 values of ``v_min``, ``v_max`` and ``sigma_ratio`` and on ``y`` as given, and
    rounded to ``y0``'s dtype once (csrc/value_rescale.h's convention; csrc/c51_head.hip ``hlg_head_kernel``).
    y is clamped, so the denominator is at least the mass of half a bin.  The mean sum_i m_i z_i is y in the
    interior and biased towards the middle within a few sigma of either end (the Gaussian is truncated there):
    priorities are taken against y, not against that mean.  y0 [B] -> m [B, N]."""
    N = int(num_atoms)
    sr = _f32(sigma_ratio)
    if not (sr > 0.0 and sr < float("inf")):
        raise ValueError(f"hl_gauss_sigma_ratio must be finite and > 0, got {sigma_ratio}")
    lo, hi = _f32(v_min), _f32(v_max)
    delta = (hi - lo) / (N - 1)
    y = y0.clamp(float(v_min), float(v_max)).double()
    edges = lo + (torch.arange(N + 1, dtype=torch.float64, device=y0.device) - 0.5) * delta
    E = torch.erf((edges[None, :] - y[:, None]) / (sr * delta * 1.4142135623730951))
    m = (E[:, 1:] - E[:, :-1]) / (E[:, -1:] - E[:, :1])
    return m.to(y0.dtype)


def hl_gauss_loss(logp_t: torch.Tensor, q_online_next: torch.Tensor, q_target_next: torch.Tensor,
                  A: torch.Tensor, R: torch.Tensor, Gamma: torch.Tensor, v_min: float, v_max: float,
                  sigma_ratio: float = 0.75, weights: torch.Tensor = None,
                  rescale_eps: float = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Histogram-loss (HL-Gauss) double-DQN loss of the categorical head.  ``logp_t`` [B, A, N]: log p(S_t) of the
    online net; ``q_online_next`` [B, A]: its expected q at S_{t+n} (picks a*, first maximum); ``q_target_next``
    [B, A]: the target net's expected q at S_{t+n}.  y0 = R + Gamma q_target[a*] (:func:`ddqn_targets`; with
    ``rescale_eps`` T(R, Gamma, q_target[a*]), fp64 on the given values and rounded once), y its clamp onto
    [v_min, v_max], m = :func:`hl_gauss_target`.  Returns (mean over the batch of -w sum_i m_i log p(S_t)[a, i],
    |y - q(S_t)[a]| per sample): the priority is the TD error against the scalar target the row was built from.
    Computes in ``logp_t``'s dtype (fp64 inputs: the tests' reference)."""
    B, _, N = logp_t.shape
    dt = logp_t.dtype
    ar = torch.arange(B, device=logp_t.device)
    with torch.no_grad():
        if rescale_eps is not None:
            y0 = ddqn_targets(q_online_next, q_target_next.to(dt).double(), R.to(dt).double(), Gamma.to(dt).double(),
                              rescale_eps).to(dt)
        else:
            y0 = ddqn_targets(q_online_next, q_target_next.to(dt), R.to(dt), Gamma.to(dt))
        y = y0.clamp(float(v_min), float(v_max))
        m = hl_gauss_target(y, v_min, v_max, N, sigma_ratio)
        delta = (float(v_max) - float(v_min)) / (N - 1)
        z = float(v_min) + torch.arange(N, dtype=dt, device=logp_t.device) * delta
    lp = logp_t[ar, A.long().view(-1)]
    per = -(m * lp).sum(-1)
    if weights is not None:
        per = per * weights.to(dt)
    with torch.no_grad():
        td = (y - (lp.exp() * z).sum(-1)).abs()
    return per.mean(), td


def quantile_huber_terms(theta: torch.Tensor, T: torch.Tensor, kappa: float,
                         tau: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The quantile Huber loss of N quantiles ``theta`` [B, N] at tau_i = (2 i + 1) / (2 N)
    (or at the given fractions ``tau`` [B, N]: the implicit quantile head's sampled ones)
    against N target samples ``T`` [B, N'], u_ij = T_j - theta_i:

        rho[b, i] = (1/N) sum_j |tau_i - 1{u_ij < 0}| L_kappa(u_ij) / kappa
        c[b, i]   = (1/N) sum_j |tau_i - 1{u_ij < 0}| clamp(u_ij, -kappa, kappa) / kappa

    so d (sum_i rho) / d theta_i = -c_i.  The j-sums run in increasing j (a fixed-order loop:
    the kernel's order); computes in ``theta``'s dtype.  ``rho`` carries theta's autograd
    graph, ``c`` is detached."""
    N = T.shape[-1]
    dt = theta.dtype
    kappa = float(kappa)
    if tau is None:
        tau = ((2.0 * torch.arange(N, dtype=dt, device=theta.device) + 1.0) / (2.0 * N))[None, :]
    else:
        tau = tau.to(dt)
    rho = torch.zeros_like(theta)
    c = torch.zeros_like(theta)
    for j in range(N):        # fixed order: the kernels' sum
        u = T[:, j:j + 1].to(dt) - theta
        wgt = (tau - (u.detach() < 0).to(dt)).abs()
        rho = rho + wgt * huber(u, kappa)
        c = c + wgt * u.detach().clamp(-kappa, kappa)
    return rho / (N * kappa), c / (N * kappa)


def quantile_targets(R: torch.Tensor, Gamma: torch.Tensor, theta: torch.Tensor,
                     rescale_eps: float = None) -> torch.Tensor:
    """The target samples T_j [B, N] of the two quantile heads from the target net's ``theta`` [B, N] of a*:
    R + Gamma theta_j, or with ``rescale_eps`` (``Runtime.value_rescale``) h(R + Gamma h^-1(theta_j)) per
    sample -- exact, the quantiles of a monotone image being the images of the quantiles."""
    if rescale_eps is not None:
        return rescale_target(R[:, None], Gamma[:, None], theta, float(rescale_eps))
    return R[:, None] + Gamma[:, None] * theta


def quantile_huber_loss(theta_t: torch.Tensor, q_online_next: torch.Tensor, theta_target_next: torch.Tensor,
                        A: torch.Tensor, R: torch.Tensor, Gamma: torch.Tensor, kappa: float,
                        weights: torch.Tensor = None, rescale_eps: float = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantile-regression (QR-DQN) double-DQN loss.  ``theta_t`` [B, A, N]: the online
    net's quantiles at S_t; ``q_online_next`` [B, A]: its q (mean of the quantiles) at
    S_{t+n}, which picks a* (first maximum); ``theta_target_next`` [B, A, N]: the target
    net's quantiles at S_{t+n}.  T_j = R + Gamma theta_target[a*, j] (Gamma = 0 at terminals
    needs no special case).  Returns (mean over the batch of w sum_i rho_i, see
    :func:`quantile_huber_terms`; |mean_j T_j - q(S_t)[a]| per sample): the priority is the
    absolute TD error of the expectations, on the scale of the actors' initial priorities.
    Computes in ``theta_t``'s dtype.  With ``rescale_eps`` the priority takes the mean of the transformed T_j
    (no longer |R + Gamma q_target[a*] - q|)."""
    B = theta_t.shape[0]
    dt = theta_t.dtype
    ar = torch.arange(B, device=theta_t.device)
    with torch.no_grad():
        a_star = q_online_next.argmax(dim=1)
        T = quantile_targets(R.to(dt), Gamma.to(dt), theta_target_next[ar, a_star].to(dt), rescale_eps)
    th = theta_t[ar, A.long().view(-1)]
    per = quantile_huber_terms(th, T, kappa)[0].sum(-1)
    if weights is not None:
        per = per * weights.to(dt)
    with torch.no_grad():
        td = (T.mean(-1) - th.mean(-1)).abs()
    return per.mean(), td


def iqn_loss(theta_t: torch.Tensor, tau_t: torch.Tensor, q_online_next: torch.Tensor,
             theta_target_next: torch.Tensor, A: torch.Tensor, R: torch.Tensor, Gamma: torch.Tensor, kappa: float,
             weights: torch.Tensor = None, rescale_eps: float = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Implicit quantile (IQN) double-DQN loss: :func:`quantile_huber_loss` with sampled
    fractions.  ``theta_t`` [B, A, N]: the online net at S_t evaluated at ``tau_t`` [B, N];
    ``q_online_next`` [B, A]: its q at S_{t+n} (the mean over its own tau set), which picks a*
    (first maximum); ``theta_target_next`` [B, A, N']: the target net at S_{t+n} at its own
    tau set (the fractions of the target samples do not enter the loss).  Returns (mean over
    the batch of w sum_i rho_i, |mean_j T_j - mean_i theta_i| per sample)."""
    B = theta_t.shape[0]
    dt = theta_t.dtype
    ar = torch.arange(B, device=theta_t.device)
    with torch.no_grad():
        a_star = q_online_next.argmax(dim=1)
        T = quantile_targets(R.to(dt), Gamma.to(dt), theta_target_next[ar, a_star].to(dt), rescale_eps)
    th = theta_t[ar, A.long().view(-1)]
    per = quantile_huber_terms(th, T, kappa, tau_t)[0].sum(-1)
    if weights is not None:
        per = per * weights.to(dt)
    with torch.no_grad():
        td = (T.mean(-1) - th.mean(-1)).abs()
    return per.mean(), td


def tau_log_policy(g: torch.Tensor, tau: float) -> torch.Tensor:
    """tau ln softmax(g / tau) over the last axis, max-subtracted: (g - max g) - tau ln sum exp((g - max g) /
    tau).  Cannot overflow; a term that underflows to 0 is the correct limit."""
    c = g - g.max(dim=-1, keepdim=True).values
    return c - float(tau) * torch.log(torch.exp(c / float(tau)).sum(dim=-1, keepdim=True))


def munchausen_targets(q_target_t: torch.Tensor, q_target_next: torch.Tensor, A: torch.Tensor, R: torch.Tensor,
                       Gamma: torch.Tensor, alpha: float, tau: float,
                       clip: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(T, bonus, vsoft) of the Munchausen-DQN target, each [B], in ``q_target_t``'s dtype:

        bonus = alpha clamp(tau ln pi(a | g0), clip, 0)            g0 = Q_target(S_t)
        vsoft = sum_a' pi(a' | g1) (g1[a'] - tau ln pi(a' | g1))   g1 = Q_target(S_t+n)
        T     = R + bonus + Gamma vsoft

    pi = softmax(g / tau).  vsoft is evaluated as the expectation (analytically max g1 + tau ln sum exp((g1 -
    max g1) / tau), the form the kernel uses).  Gamma = 0 at terminals needs no special case; with n-step
    returns the bonus is paid on the first transition only."""
    dt = q_target_t.dtype
    g0, g1 = q_target_t, q_target_next.to(dt)
    tl0 = tau_log_policy(g0, tau).gather(1, A.long().view(-1, 1)).squeeze(1)
    bonus = float(alpha) * tl0.clamp(float(clip), 0.0)
    tl1 = tau_log_policy(g1, tau)
    vsoft = ((tl1 / float(tau)).exp() * (g1 - tl1)).sum(-1)
    return R.to(dt) + bonus + Gamma.to(dt) * vsoft, bonus, vsoft


def munchausen_loss(q_t: torch.Tensor, q_target_t: torch.Tensor, q_target_next: torch.Tensor, A: torch.Tensor,
                    R: torch.Tensor, Gamma: torch.Tensor, w: torch.Tensor = None, alpha: float = 0.9,
                    tau: float = 0.03, clip: float = -1.0, loss: str = "huber",
                    kappa: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Munchausen-DQN loss (Vieillard, Pietquin, Geist 2020) of the scalar head: ``q_t`` [B, A] the online
    net at S_t, ``q_target_t`` / ``q_target_next`` the target net at S_t / S_t+n.  delta = T - q_t[a] with T
    of :func:`munchausen_targets` (no online argmax: this is not double DQN), the Huber or 0.5 delta^2 loss
    weighted by ``w``; the gradient flows through q_t[a] only.  Returns (scalar loss, |delta| per sample) as
    :func:`ddqn_loss`; computes in ``q_t``'s dtype (fp64 inputs: the tests' reference)."""
    dt = q_t.dtype
    with torch.no_grad():
        T = munchausen_targets(q_target_t.to(dt), q_target_next.to(dt), A, R, Gamma, alpha, tau, clip)[0]
    q_sa = q_t.gather(1, A.long().view(-1, 1)).squeeze(1)
    delta = T - q_sa
    per = huber(delta, kappa) if loss == "huber" else 0.5 * delta * delta
    if w is not None:
        per = per * w.to(dt)
    return per.mean(), delta.detach().abs()


def ddqn_loss(q_online_t: torch.Tensor, q_online_next: torch.Tensor,
              q_target_next: torch.Tensor, A: torch.Tensor, R: torch.Tensor,
              Gamma: torch.Tensor, weights: torch.Tensor = None, loss: str = "huber",
              kappa: float = 1.0, rescale_eps: float = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Return (scalar loss, |delta| per sample).  ``rescale_eps``: the rescaled target of :func:`ddqn_targets`
    (fp64 on the fp32 inputs, rounded to fp32 once: the kernel's evaluation)."""
    with torch.no_grad():
        if rescale_eps is not None:
            G = ddqn_targets(q_online_next.float().double(), q_target_next.float().double(), R.float().double(),
                             Gamma.float().double(), rescale_eps).float()
        else:
            G = ddqn_targets(q_online_next.float(), q_target_next.float(), R.float(), Gamma.float())
    q_sa = q_online_t.float().gather(1, A.long().view(-1, 1)).squeeze(1)
    delta = G - q_sa
    per = huber(delta, kappa) if loss == "huber" else 0.5 * delta * delta
    if weights is not None:
        per = per * weights.float()
    return per.mean(), delta.detach().abs()
