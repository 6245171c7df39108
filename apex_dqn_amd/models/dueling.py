"""Dueling Q-networks (PyTorch reference implementations).

These modules are the *semantic* definition of every network family and the
CPU / oracle path.  The MI355X training paths (``learner/fused_learner.py``
for the NatureCNN, ``learner/impala_learner.py`` for IMPALA-deep) run the same
math through hand-written HIP kernels on a flat parameter buffer
(``models/flat_params.py``) and convert to/from these modules' ``state_dict``
so checkpoints stay interchangeable.

``DuellingDQN`` keeps the reference key names exactly
(``duelling_network.py:8-19``: ``layer1.0.weight`` ... ``advantage.bias``)
so ``torch.load(p)['Q_state']`` checkpoints load unchanged, and keeps the
``forward -> (value, advantage, q)`` contract (``duelling_network.py:28``).

Deliberate deviation: the advantage mean is taken per
sample (``adv.mean(1)``), not over the whole batch tensor as in
``duelling_network.py:27``.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F


def dueling_combine(value: torch.Tensor, adv: torch.Tensor) -> torch.Tensor:
    """q = v + a - mean_a(a), per sample."""
    return value + adv - adv.mean(dim=1, keepdim=True)


class NoisyLinear(nn.Module):
    """Linear layer with factorised Gaussian noise (Fortunato et al. 2018):
    W = mu_w + sigma_w * (xi_out (x) xi_in), b = mu_b + sigma_b * xi_out.  ``weight`` / ``bias``
    keep ``nn.Linear``'s names, shapes and default init (U(-1/sqrt(p), 1/sqrt(p)), p the
    fan-in) and hold mu; ``weight_sigma`` / ``bias_sigma`` start at sigma0 / sqrt(p).  The
    noise is injected (:meth:`set_noise`; learner/noisy.py ``noise_vectors``), never drawn
    here: the learner, the oracle and the kernels see one draw.  No noise set = zero noise."""

    def __init__(self, in_features: int, out_features: int, sigma0: float = 0.5):
        super().__init__()
        self.in_features, self.out_features = int(in_features), int(out_features)
        lin = nn.Linear(self.in_features, self.out_features)     # (the same RNG use as the plain layer)
        self.weight = nn.Parameter(lin.weight.detach().clone())
        self.bias = nn.Parameter(lin.bias.detach().clone())
        s = float(sigma0) / float(self.in_features) ** 0.5
        self.weight_sigma = nn.Parameter(torch.full((self.out_features, self.in_features), s))
        self.bias_sigma = nn.Parameter(torch.full((self.out_features,), s))
        self.register_buffer("xi_in", torch.zeros(self.in_features), persistent=False)
        self.register_buffer("xi_out", torch.zeros(self.out_features), persistent=False)

    def set_noise(self, xi_out: torch.Tensor, xi_in: torch.Tensor) -> None:
        with torch.no_grad():
            self.xi_out.copy_(xi_out.reshape(-1).to(self.xi_out.dtype))
            self.xi_in.copy_(xi_in.reshape(-1).to(self.xi_in.dtype))

    def effective(self):
        w = self.weight + self.weight_sigma * torch.outer(self.xi_out, self.xi_in)
        return w, self.bias + self.bias_sigma * self.xi_out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        w, b = self.effective()
        return F.linear(x, w, b)


def _linear(p: int, rows: int, noisy: bool, sigma0: float) -> nn.Module:
    return NoisyLinear(p, rows, sigma0) if noisy else nn.Linear(p, rows)


class _C51Head:
    """Distributional (C51) dueling head shared by the modules that take ``num_atoms``:
    the value head has N outputs, the advantage head A N (row a N + i = action a, atom i),
    the dueling combine runs per atom and q is the expectation over the fixed support
    z_i = v_min + i (v_max - v_min) / (N - 1).  N = 1: the scalar head.

    ``dist_head = "quantile"`` (QR-DQN): the same weights, keys and shapes, read as N
    quantiles per action, theta[a, i] = v[i] + adv[a, i] - mean_a' adv[a', i] at tau_i =
    (2 i + 1) / (2 N); q is their mean; no support buffer (v_min / v_max are ignored).

    ``dist_head = "hl_gauss"`` (the histogram loss, learner/losses.py ``hl_gauss_loss``) changes the training
    target only: the module is the categorical one (log-probabilities, the expectation, noisy layers)."""

    def _init_head(self, hidden: int, num_atoms: int, v_min: float, v_max: float,
                   dist_head: str = "categorical", noisy: bool = False, sigma0: float = 0.5,
                   iqn_actor_samples: int = 32) -> None:
        if dist_head not in ("categorical", "quantile", "implicit", "hl_gauss"):
            raise ValueError(f"dist_head must be 'categorical', 'quantile', 'implicit' or 'hl_gauss', got "
                             f"{dist_head!r}")
        self.num_atoms = int(num_atoms)
        # "hl_gauss" (the histogram loss) is another target for the categorical head: the module is the same
        self.dist_head = dist_head if self.num_atoms > 1 and dist_head != "hl_gauss" else "categorical"
        self.v_min, self.v_max = float(v_min), float(v_max)
        self.noisy = bool(noisy)
        self.implicit = self.dist_head == "implicit"
        if self.implicit and self.noisy:
            raise ValueError("dist_head 'implicit' has no noisy layers")
        # implicit (IQN): the heads at the scalar head's shapes; num_atoms is the loss's sample count only
        rows = 1 if self.implicit else self.num_atoms
        self.value = _linear(hidden, rows, self.noisy, sigma0)
        self.advantage = _linear(hidden, self.action_dim * rows, self.noisy, sigma0)
        if self.implicit:
            # the cosine embedding of tau (64 cosines, the paper's n) gating both stream activations
            self.tau_embed = nn.Linear(64, 2 * hidden)
            self.iqn_actor_samples = int(iqn_actor_samples)
            # (seed_q, counter word) of the next forward's K fractions per row, set by an actor group's hook
            # (learner/iqn.py actor_tau_hook); None: the greedy evaluation's midpoints
            self.iqn_draw = None
        if self.num_atoms > 1 and self.dist_head == "categorical":
            self.register_buffer("support", c51_support(self.num_atoms, self.v_min, self.v_max), persistent=False)

    def set_noise(self, v) -> None:
        """Inject one network draw (learner/noisy.py ``noise_vectors``: ``fc_in_v``, ``fc_in_a``,
        ``fc_out``, ``v_in``, ``a_in``, ``v_out``, ``a_out``) into the four noisy layers.  The
        stream layers' xi_in comes in the engine's h, w, c column order (models/flat_params.py)
        and is permuted to this module's c, h, w order; an MLP's columns are used as given."""
        assert self.noisy, "set_noise on a network without noisy layers"
        lv, la = self.value_stream_layer[0], self.advantage_stream_layer[0]
        h = lv.out_features

        def cols(x):
            if x.numel() == 3136 and len(self.input_shape) == 3:
                return x.reshape(7, 7, 64).permute(2, 0, 1).reshape(-1)
            return x

        lv.set_noise(v["fc_out"][:h], cols(v["fc_in_v"]))
        la.set_noise(v["fc_out"][h:], cols(v["fc_in_a"]))
        self.value.set_noise(v["v_out"], v["v_in"])
        self.advantage.set_noise(v["a_out"], v["a_in"])

    def _head(self, hv: torch.Tensor, ha: torch.Tensor):
        """(value, advantage, q, dist): dist = [B, A, N] log-probabilities (categorical) or
        quantiles (quantile); None for the scalar head."""
        if self.implicit:
            # q = the mean over K fractions: an actor's draws (row e of the call, index e 64 + k), or for the
            # greedy evaluation the midpoints tau_k = (2 k + 1) / (2 K)
            from ..learner.iqn import midpoint_taus, stream_taus
            if self.iqn_draw is not None:
                tau = stream_taus(self.iqn_draw[0], self.iqn_draw[1], hv.shape[0], self.iqn_actor_samples).to(hv.device)
            else:
                tau = midpoint_taus(self.iqn_actor_samples).to(hv.device)[None, :].expand(hv.shape[0], -1)
            theta, v, adv = self._theta_at(hv, ha, tau)
            return v.mean(1, keepdim=True), adv.mean(1), theta.mean(-1), theta
        value, advantage = self.value(hv), self.advantage(ha)
        if self.num_atoms == 1:
            return value, advantage, dueling_combine(value, advantage), None
        if self.dist_head == "quantile":
            theta = dueling_quantiles(value, advantage, self.action_dim)
            return value, advantage, theta.mean(-1), theta
        logp = c51_log_probs(value, advantage, self.action_dim)
        q = (logp.exp() * self.support.to(logp.dtype)).sum(-1)
        return value, advantage, q, logp

    def _theta_at(self, hv: torch.Tensor, ha: torch.Tensor, tau: torch.Tensor):
        """theta [rows, A, n], v [rows, n], adv [rows, n, A] at the fractions ``tau`` [rows, n]: c_i = cos(pi i
        tau) (fp64 at the given tau, then cast), phi = relu(We c + be), x = h * phi, v = wv . x[:H] + bv, adv_a
        = wa[a] . x[H:] + ba[a], theta[a] = v + adv_a - mean_a' adv_a'."""
        from ..learner.iqn import cos_features
        H = hv.shape[-1]
        phi = F.relu(self.tau_embed(cos_features(tau, hv.dtype).to(hv.device)))
        v = self.value(hv[:, None, :] * phi[..., :H]).squeeze(-1)
        adv = self.advantage(ha[:, None, :] * phi[..., H:])
        theta = v[..., None] + adv - adv.mean(-1, keepdim=True)
        return theta.transpose(1, 2), v, adv

    def quantiles_at(self, x: torch.Tensor, tau: torch.Tensor) -> torch.Tensor:
        """[rows, A, n] quantile values of the implicit head at the fractions ``tau`` [rows, n]."""
        assert self.implicit
        return self._theta_at(*self.streams(x), tau)[0]


def c51_support(num_atoms: int, v_min: float, v_max: float, dtype=torch.float32) -> torch.Tensor:
    """z_i = v_min + i (v_max - v_min) / (N - 1), evaluated in fp64 and rounded to ``dtype``."""
    delta = (float(v_max) - float(v_min)) / (int(num_atoms) - 1)
    return (float(v_min) + torch.arange(int(num_atoms), dtype=torch.float64) * delta).to(dtype)


def c51_log_probs(value: torch.Tensor, advantage: torch.Tensor, action_dim: int) -> torch.Tensor:
    """[B, A, N] log-probabilities: per-atom dueling combine, log-softmax over the atoms."""
    B, N = value.shape
    adv = advantage.reshape(B, action_dim, N)
    logits = value[:, None, :] + adv - adv.mean(dim=1, keepdim=True)
    return F.log_softmax(logits, dim=-1)


def dueling_quantiles(value: torch.Tensor, advantage: torch.Tensor, action_dim: int) -> torch.Tensor:
    """[B, A, N] quantiles theta[a, i] = v[i] + adv[a, i] - mean_a' adv[a', i] (the dueling
    mean per quantile)."""
    B, N = value.shape
    adv = advantage.reshape(B, action_dim, N)
    return value[:, None, :] + adv - adv.mean(dim=1, keepdim=True)


class _ObsScale(nn.Module):
    def __init__(self, scale: float):
        super().__init__()
        self.scale = float(scale)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype == torch.uint8:
            return x.float() * self.scale
        return x.float() if not x.is_floating_point() else x


class DuellingDQN(nn.Module, _C51Head):
    """Dueling NatureCNN: 3 conv + two 512-wide streams + value/advantage heads.

    ``conv1_channels`` = 64 matches the reference checkpoint layout
    (``duelling_network.py:8``); 32 gives the Nature/dueling-paper variant.
    uint8 input is scaled by ``obs_scale`` (1/255 by default); float input is
    used as given (the reference feeds raw 0..255 floats).
    """

    def __init__(self, state_shape: Sequence[int], action_dim: int,
                 conv1_channels: int = 64, obs_scale: float = 1.0 / 255.0,
                 num_atoms: int = 1, v_min: float = -10.0, v_max: float = 10.0,
                 dist_head: str = "categorical", noisy: bool = False, noisy_sigma0: float = 0.5,
                 iqn_actor_samples: int = 32):
        super().__init__()
        self.input_shape = tuple(state_shape)
        self.action_dim = int(action_dim)
        c = int(state_shape[0])
        c1 = int(conv1_channels)
        self.pre = _ObsScale(obs_scale)
        self.layer1 = nn.Sequential(nn.Conv2d(c, c1, 8, stride=4), nn.ReLU())
        self.layer2 = nn.Sequential(nn.Conv2d(c1, 64, 4, stride=2), nn.ReLU())
        self.layer3 = nn.Sequential(nn.Conv2d(64, 64, 3, stride=1), nn.ReLU())
        self.value_stream_layer = nn.Sequential(_linear(64 * 7 * 7, 512, noisy, noisy_sigma0), nn.ReLU())
        self.advantage_stream_layer = nn.Sequential(_linear(64 * 7 * 7, 512, noisy, noisy_sigma0), nn.ReLU())
        self._init_head(512, num_atoms, v_min, v_max, dist_head, noisy, noisy_sigma0, iqn_actor_samples)

    def streams(self, x: torch.Tensor):
        h = self.features(x)
        return self.value_stream_layer(h), self.advantage_stream_layer(h)

    def features(self, x: torch.Tensor) -> torch.Tensor:
        x = self.pre(x)
        x = self.layer3(self.layer2(self.layer1(x)))
        return x.reshape(x.shape[0], -1)

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        h = self.features(x)
        return self._head(self.value_stream_layer(h), self.advantage_stream_layer(h))[:3]

    def log_probs(self, x: torch.Tensor) -> torch.Tensor:
        """[B, A, N] log-probabilities of the value distribution (``num_atoms`` >= 2)."""
        assert self.dist_head == "categorical" and self.num_atoms > 1
        h = self.features(x)
        return self._head(self.value_stream_layer(h), self.advantage_stream_layer(h))[3]

    def quantiles(self, x: torch.Tensor) -> torch.Tensor:
        """[B, A, N] quantiles of the value distribution (``dist_head = "quantile"``)."""
        assert self.dist_head == "quantile"
        h = self.features(x)
        return self._head(self.value_stream_layer(h), self.advantage_stream_layer(h))[3]


class MLPDuellingDQN(nn.Module, _C51Head):
    """Dueling MLP for low-dimensional states (CartPole config)."""

    def __init__(self, state_shape: Sequence[int], action_dim: int, hidden: int = 128,
                 num_atoms: int = 1, v_min: float = -10.0, v_max: float = 10.0,
                 dist_head: str = "categorical", noisy: bool = False, noisy_sigma0: float = 0.5,
                 iqn_actor_samples: int = 32):
        super().__init__()
        d = int(state_shape[0]) if len(state_shape) == 1 else int(torch.tensor(state_shape).prod())
        self.input_shape = tuple(state_shape)
        self.action_dim = int(action_dim)
        self.layer1 = nn.Sequential(nn.Linear(d, hidden), nn.ReLU())
        self.value_stream_layer = nn.Sequential(_linear(hidden, hidden, noisy, noisy_sigma0), nn.ReLU())
        self.advantage_stream_layer = nn.Sequential(_linear(hidden, hidden, noisy, noisy_sigma0), nn.ReLU())
        self._init_head(hidden, num_atoms, v_min, v_max, dist_head, noisy, noisy_sigma0, iqn_actor_samples)

    def streams(self, x: torch.Tensor):
        h = self.layer1(x.float().reshape(x.shape[0], -1))
        return self.value_stream_layer(h), self.advantage_stream_layer(h)

    def forward(self, x: torch.Tensor):
        h = self.layer1(x.float().reshape(x.shape[0], -1))
        return self._head(self.value_stream_layer(h), self.advantage_stream_layer(h))[:3]

    def log_probs(self, x: torch.Tensor) -> torch.Tensor:
        """[B, A, N] log-probabilities of the value distribution (``num_atoms`` >= 2)."""
        assert self.dist_head == "categorical" and self.num_atoms > 1
        h = self.layer1(x.float().reshape(x.shape[0], -1))
        return self._head(self.value_stream_layer(h), self.advantage_stream_layer(h))[3]

    def quantiles(self, x: torch.Tensor) -> torch.Tensor:
        """[B, A, N] quantiles of the value distribution (``dist_head = "quantile"``)."""
        assert self.dist_head == "quantile"
        h = self.layer1(x.float().reshape(x.shape[0], -1))
        return self._head(self.value_stream_layer(h), self.advantage_stream_layer(h))[3]


class _ResBlock(nn.Module):
    def __init__(self, ch: int):
        super().__init__()
        self.conv0 = nn.Conv2d(ch, ch, 3, padding=1)
        self.conv1 = nn.Conv2d(ch, ch, 3, padding=1)

    def forward(self, x):
        y = self.conv0(F.relu(x))
        y = self.conv1(F.relu(y))
        return x + y


class _ImpalaStack(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, padding=1)
        self.res0 = _ResBlock(cout)
        self.res1 = _ResBlock(cout)

    def forward(self, x):
        x = self.conv(x)
        x = F.max_pool2d(x, 3, stride=2, padding=1)
        return self.res1(self.res0(x))


class ImpalaDuellingDQN(nn.Module):
    """IMPALA-deep ResNet trunk (16/32/32 channels) with dueling heads.

    BASELINE.json config 5 ("IMPALA-deep ResNet dueling Q-net on Atari"); not
    present in the reference.
    """

    def __init__(self, state_shape: Sequence[int], action_dim: int,
                 channels: Sequence[int] = (16, 32, 32), hidden: int = 256,
                 obs_scale: float = 1.0 / 255.0):
        super().__init__()
        c, h, w = (int(s) for s in state_shape)
        self.input_shape = (c, h, w)
        self.action_dim = int(action_dim)
        self.pre = _ObsScale(obs_scale)
        stacks = []
        cin = c
        for ch in channels:
            stacks.append(_ImpalaStack(cin, ch))
            cin = ch
            h, w = (h + 1) // 2, (w + 1) // 2
        self.stacks = nn.ModuleList(stacks)
        flat = cin * h * w
        self.value_stream_layer = nn.Sequential(nn.Linear(flat, hidden), nn.ReLU())
        self.advantage_stream_layer = nn.Sequential(nn.Linear(flat, hidden), nn.ReLU())
        self.value = nn.Linear(hidden, 1)
        self.advantage = nn.Linear(hidden, self.action_dim)

    def forward(self, x):
        x = self.pre(x)
        for s in self.stacks:
            x = s(x)
        hcat = F.relu(x).reshape(x.shape[0], -1)
        value = self.value(self.value_stream_layer(hcat))
        advantage = self.advantage(self.advantage_stream_layer(hcat))
        return value, advantage, dueling_combine(value, advantage)


def build_network(kind: str, state_shape: Sequence[int], action_dim: int,
                  obs_scale: float = 1.0 / 255.0, num_atoms: int = 1, v_min: float = -10.0,
                  v_max: float = 10.0, dist_head: str = "categorical", noisy: bool = False,
                  noisy_sigma0: float = 0.5, iqn_actor_samples: int = 32) -> nn.Module:
    head = dict(num_atoms=num_atoms, v_min=v_min, v_max=v_max, dist_head=dist_head, noisy=noisy,
                noisy_sigma0=noisy_sigma0, iqn_actor_samples=iqn_actor_samples)
    if kind == "nature64":
        return DuellingDQN(state_shape, action_dim, conv1_channels=64, obs_scale=obs_scale, **head)
    if kind == "nature32":
        return DuellingDQN(state_shape, action_dim, conv1_channels=32, obs_scale=obs_scale, **head)
    if kind == "mlp":
        return MLPDuellingDQN(state_shape, action_dim, **head)
    if kind == "impala":
        if int(num_atoms) != 1:
            raise ValueError("Runtime.num_atoms >= 2: the impala network has no distributional head")
        if noisy:
            raise ValueError("Runtime.noisy: the impala network has no noisy layers")
        return ImpalaDuellingDQN(state_shape, action_dim, obs_scale=obs_scale)
    raise ValueError(f"unknown network kind {kind!r}")


REFERENCE_KEYS = (
    "layer1.0.weight", "layer1.0.bias", "layer2.0.weight", "layer2.0.bias",
    "layer3.0.weight", "layer3.0.bias",
    "value_stream_layer.0.weight", "value_stream_layer.0.bias",
    "advantage_stream_layer.0.weight", "advantage_stream_layer.0.bias",
    "value.weight", "value.bias", "advantage.weight", "advantage.bias",
)
NOISY_LAYERS = ("value_stream_layer.0", "advantage_stream_layer.0", "value", "advantage")
SIGMA_KEYS = tuple(f"{l}.{p}_sigma" for l in NOISY_LAYERS for p in ("weight", "bias"))
