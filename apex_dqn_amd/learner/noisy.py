"""Factorised NoisyNet layers (Fortunato et al. 2018): the noise draw's host mirror and
the index plan shared by the module (models/dueling.py ``NoisyLinear``), the torch
backend's oracle and the kernels (csrc/noisy.hip).

One network draw is ONE concatenated vector xi indexed by k, in this order:

  xi_in  of the value-stream fc       3136   (the engine's h, w, c column order)
  xi_in  of the advantage-stream fc   3136
  xi_out of the fc                    1024   (the engine's ``wfc`` row order)
  xi_in  of the value head             512
  xi_in  of the advantage head         512
  xi_out of the value head               N
  xi_out of the advantage head         A N

keyed by a stream ``s`` (0 learner online, 1 learner target, 2 + g actor group g) and an
index ``u`` (the learner's update index / the actor's inference-call index):

  c  = 64 u + s
  u1 = 1 - apex_uniform(seed_n, c, 2 k),   u2 = apex_uniform(seed_n, c, 2 k + 1)
  g  = sqrt(-2 ln u1) cos(2 pi u2),        xi = sign(g) sqrt(|g|)

``apex_uniform`` is the replay's counter RNG (csrc/apex_common.h, replay/gpu_replay.py).
The mirror evaluates g in fp64 from the fp32 uniforms; the kernel evaluates it in fp32.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from ..replay.gpu_replay import _mix64, apex_uniform

FC_IN, FC_OUT, HEAD_IN = 3136, 1024, 512
STREAMS_PER_INDEX = 64      # c = 64 u + s: streams 0 / 1 the learner's nets, 2 + g actor group g
MU = ("wv", "bv", "wa", "ba", "wfc", "bfc")
SIGMA = {"wv": "swv", "bv": "sbv", "wa": "swa", "ba": "sba", "wfc": "swfc", "bfc": "sbfc"}


def noise_seed(seed: int) -> int:
    """seed_n of ``Runtime.seed``: a mixed word, so the noise stream never coincides with the
    replay's sampling stream (which is seeded by ``Runtime.seed`` and small offsets of it)."""
    with np.errstate(over="ignore"):
        return int(_mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64(0x4E6F697379))) & ((1 << 63) - 1)


def xi_offsets(A: int, N: int, hidden: int = HEAD_IN, fc_in: int = FC_IN) -> Dict[str, int]:
    """Offsets of the seven parts in the concatenated draw, plus its length ``K``."""
    fc_out = 2 * hidden
    o, off = 0, {}
    for name, n in (("fc_in_v", fc_in), ("fc_in_a", fc_in), ("fc_out", fc_out), ("v_in", hidden), ("a_in", hidden),
                    ("v_out", int(N)), ("a_out", int(A) * int(N))):
        off[name] = o
        o += n
    off["K"] = o
    return off


def gaussians(seed: int, u: int, s: int, K: int) -> np.ndarray:
    """The K standard normal draws of (seed, u, s), fp64 (Box-Muller on the fp32 uniforms)."""
    c = STREAMS_PER_INDEX * int(u) + int(s)
    k = np.arange(int(K), dtype=np.uint64)
    u1 = 1.0 - apex_uniform(seed, c, 2 * k).astype(np.float64)
    u2 = apex_uniform(seed, c, 2 * k + 1).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def xi_of(g: np.ndarray) -> np.ndarray:
    return np.sign(g) * np.sqrt(np.abs(g))


def noise_vectors(seed: int, u: int, s: int, A: int, N: int, hidden: int = HEAD_IN,
                  fc_in: int = FC_IN) -> Dict[str, torch.Tensor]:
    """The draw (seed, u, s) as named fp64 vectors (the keys of :func:`xi_offsets`) plus the
    concatenation under ``"xi"``.  ``seed`` is seed_n (:func:`noise_seed`)."""
    off = xi_offsets(A, N, hidden, fc_in)
    xi = torch.from_numpy(xi_of(gaussians(seed, u, s, off["K"])))
    return split_xi(xi, A, N, hidden, fc_in)


def split_xi(xi: torch.Tensor, A: int, N: int, hidden: int = HEAD_IN, fc_in: int = FC_IN) -> Dict[str, torch.Tensor]:
    """Named views of a concatenated draw."""
    off = xi_offsets(A, N, hidden, fc_in)
    names = [k for k in off if k != "K"]
    ends = [off[n] for n in names[1:]] + [off["K"]]
    out = {n: xi[off[n]:e] for n, e in zip(names, ends)}
    out["xi"] = xi[:off["K"]]
    return out


def layer_noise(v: Dict[str, torch.Tensor]) -> Dict[str, tuple]:
    """(xi_out, xi_in) of the heads' weights and (xi_out, None) of the noisy biases, per flat mu
    segment (``wfc`` has one xi_in per stream: :func:`outer`)."""
    return {"wv": (v["v_out"], v["v_in"]), "wa": (v["a_out"], v["a_in"]), "bv": (v["v_out"], None),
            "ba": (v["a_out"], None), "bfc": (v["fc_out"], None)}


def outer(v: Dict[str, torch.Tensor], name: str, shape) -> torch.Tensor:
    """xi_out (x) xi_in of the mu segment ``name`` in the segment's own shape (biases: xi_out)."""
    if name == "wfc":
        h = v["fc_out"].numel() // 2
        return torch.cat([torch.outer(v["fc_out"][:h], v["fc_in_v"]), torch.outer(v["fc_out"][h:], v["fc_in_a"])])
    o, i = layer_noise(v)[name]
    return (o if i is None else torch.outer(o, i)).reshape(shape)


@dataclass
class NoisyPlan:
    """What a compose / sigma-gradient launch needs to know of a learner or an actor group:
    the head's shape, the flat offsets of the six mu segments and of their sigma segments
    (models/flat_params.py ``nature_segments(noisy=True)``), the noise seed and the device
    words of the draw index: u = (ctr - base) // every (``base`` None: 0)."""
    A: int
    N: int
    offsets: Dict[str, int]
    seed: int
    ctr: torch.Tensor
    base: Optional[torch.Tensor] = None
    every: int = 1
    stream0: int = 0            # net i of a launch draws with stream s = stream0 + i

    @property
    def K(self) -> int:
        return xi_offsets(self.A, self.N)["K"]

    def index(self) -> int:
        """u, read back from the device (the torch backend; tests)."""
        c = int(self.ctr.reshape(-1)[0].item()) - (0 if self.base is None else int(self.base.reshape(-1)[0].item()))
        return max(c, 0) // int(self.every)

    def shapes(self) -> Dict[str, tuple]:
        return {"wv": (self.N, HEAD_IN), "bv": (self.N,), "wa": (self.A * self.N, HEAD_IN), "ba": (self.A * self.N,),
                "wfc": (FC_OUT, FC_IN), "bfc": (FC_OUT,)}

    def seg(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        """The segment ``name`` (mu or sigma) of a flat buffer, in its 2-D / 1-D shape."""
        mu = name if name in SIGMA else next(m for m, s in SIGMA.items() if s == name)
        shape = self.shapes()[mu]
        n = int(np.prod(shape))
        o = self.offsets[name]
        return flat[o:o + n].view(shape)


def set_module_noise(net, seed: int, u: int, s: int) -> None:
    """Inject the draw (``Runtime.seed`` = ``seed``, u, s) into a noisy dueling module
    (models/dueling.py ``set_noise``), sized by the module's own layers."""
    hidden = net.value.in_features
    v = noise_vectors(noise_seed(seed), u, s, net.action_dim, net.num_atoms, hidden,
                      net.value_stream_layer[0].in_features)
    net.set_noise(v)


def actor_stream(group: int) -> int:
    """Stream s of actor group ``group`` (2 + g, folded into the 62 actor streams)."""
    return 2 + int(group) % (STREAMS_PER_INDEX - 2)


def actor_noise_hook(cfg, net, group: int):
    """``hook(t)`` for an actor group's policy network: before inference call ``t`` it injects
    the draw (s = 2 + group, u = t // Runtime.noisy_actor_resample); None without noisy layers."""
    rt = cfg.Runtime
    if not rt.noisy:
        return None
    every, s, last = int(rt.noisy_actor_resample), actor_stream(group), [-1]

    def hook(t: int) -> None:
        u = int(t) // every
        if u != last[0]:
            set_module_noise(net, rt.seed, u, s)
            last[0] = u
    return hook
