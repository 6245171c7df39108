"""Implicit quantile networks (Dabney et al. 2018): the host mirror of the tau draws and the
cosine embedding shared by the torch oracles (ops/fused_ops.py ``iqn_head``), the module
(models/dueling.py ``quantiles_at``) and the kernels (csrc/iqn_head.hip).

Nothing is drawn from a kernel's private state: every fraction is

  tau = apex_uniform(seed_q, c, idx)        in [0, 1), tau = 0 is legal

with ``apex_uniform`` the replay's counter RNG (csrc/apex_common.h, replay/gpu_replay.py) and
``seed_q`` a mixed word of ``Runtime.seed`` (:func:`iqn_seed`), never the noise seed's.

  learner, update u:           c = 64 u,                    idx = (3 b + set) 64 + k
  actor group g, call t:       c = 64 t + actor_stream(g),  idx = e 64 + k
  greedy evaluation:           tau_k = (2 k + 1) / (2 K)    (no draw)

b is the row in the batch and ``set`` one of 0 (online net at S_t), 1 (online net at S_t+n:
picks a*), 2 (target net at S_t+n: the target samples).  The cosine feature is the fp64
value of cos(pi i tau) at the fp32 tau, i = 0..63.
"""
from __future__ import annotations

import numpy as np
import torch

from ..replay.gpu_replay import _mix64, apex_uniform
from .noisy import STREAMS_PER_INDEX, actor_stream

EMBED = 64          # cosines of the embedding (the paper's n = 64): a constant, not a key
MAX_SAMPLES = 64    # one lane per sample; also the stride of a row's draws
SETS = 3


def iqn_seed(seed: int) -> int:
    """seed_q of ``Runtime.seed``: mixed with its own constant, so the tau stream coincides
    neither with the replay's sampling stream nor with the noise stream."""
    with np.errstate(over="ignore"):
        return int(_mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64(0x49514E746175))) & ((1 << 63) - 1)


def learner_taus(seed: int, u: int, B: int, N: int) -> torch.Tensor:
    """[B, 3, N] float32: the three tau sets of every batch row at update ``u`` (``seed`` is
    seed_q)."""
    assert 1 <= int(N) <= MAX_SAMPLES
    row = np.arange(int(B) * SETS, dtype=np.uint64)[:, None] * np.uint64(MAX_SAMPLES)
    idx = row + np.arange(int(N), dtype=np.uint64)[None, :]
    t = apex_uniform(seed, STREAMS_PER_INDEX * int(u), idx)
    return torch.from_numpy(t.reshape(int(B), SETS, int(N)).copy())


def actor_taus(seed: int, t: int, group: int, E: int, K: int) -> torch.Tensor:
    """[E, K] float32: the K fractions of every env row of actor group ``group`` at its
    inference call ``t``."""
    return stream_taus(seed, STREAMS_PER_INDEX * int(t) + actor_stream(group), E, K)


def stream_taus(seed: int, c: int, E: int, K: int) -> torch.Tensor:
    """[E, K] float32 fractions of the counter word ``c`` (what ``iqn_actor_head_kernel`` draws)."""
    assert 1 <= int(K) <= MAX_SAMPLES
    idx = np.arange(int(E), dtype=np.uint64)[:, None] * np.uint64(MAX_SAMPLES) + np.arange(int(K), dtype=np.uint64)
    return torch.from_numpy(apex_uniform(seed, int(c), idx).reshape(int(E), int(K)).copy())


def midpoint_taus(K: int, dtype=torch.float32) -> torch.Tensor:
    """tau_k = (2 k + 1) / (2 K), evaluated in fp32 as the kernel does (then cast)."""
    k = torch.arange(int(K), dtype=torch.float32)
    return ((2.0 * k + 1.0) / (2.0 * float(K))).to(dtype)


def cos_features(tau: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[..., 64] cos(pi i tau): evaluated in fp64 at the given (fp32) tau, then cast."""
    i = torch.arange(EMBED, dtype=torch.float64, device=tau.device)
    return torch.cos(np.pi * tau.double()[..., None] * i).to(dtype)


def actor_tau_hook(cfg, net, group: int):
    """``hook(t)`` for an actor group's policy network on the CPU path (the inline loop, actor processes): before
    inference call ``t`` it names the draw (c = 64 t + actor_stream(group)) whose K fractions per env row the
    module's forward then uses -- the fractions ``iqn_actor_head_kernel`` draws for a GPU actor group; None without
    the implicit head."""
    if not cfg.implicit:
        return None
    seed_q, s = iqn_seed(cfg.Runtime.seed), actor_stream(group)

    def hook(t: int) -> None:
        net.iqn_draw = (seed_q, STREAMS_PER_INDEX * int(t) + s)
    return hook
