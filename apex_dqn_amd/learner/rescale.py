"""Invertible value rescaling of the n-step target (``Runtime.value_rescale``): the host mirror of
csrc/value_rescale.h and the one place the formulae are written in Python.

Pohlen et al. 2018 ("Observe and Look Further"; R2D2 uses eps = 1e-3): the network learns ``h(Q)`` for a
squashing, strictly increasing ``h`` and the target is ``h(R + Gamma h^-1(Q_target))``::

    h(x)     = sign(x) (sqrt(|x| + 1) - 1) + eps x
    h^-1(y)  = sign(y) (((sqrt(1 + 4 eps (|y| + 1 + eps)) - 1) / (2 eps))^2 - 1)
    T(R,G,y) = h(R + G h^-1(y))

``Gamma = 0`` at terminals gives ``T = h(R)`` with no special case.  Every function takes torch tensors,
numpy arrays or Python scalars and computes in the dtype of what it is given (fp64 is the reference: the
kernels evaluate fp64 on their fp32 inputs and round to fp32 once).
"""
from __future__ import annotations

import numpy as np
import torch


def check_eps(eps: float) -> float:
    eps = float(eps)
    if not 0.0 < eps <= 1.0:
        raise ValueError(f"value_rescale_eps must be in (0, 1], got {eps}")
    return eps


def _ops(x):
    if isinstance(x, torch.Tensor):
        return torch.sign, torch.abs, torch.sqrt
    return np.sign, np.abs, np.sqrt


def _arr(x):
    return x if isinstance(x, (torch.Tensor, np.ndarray)) else np.float64(x)


def h(x, eps: float = 1e-3):
    """``sign(x) (sqrt(|x| + 1) - 1) + eps x``, evaluated without the cancelling difference: ``sqrt(1 + a) - 1 =
    a / (sqrt(1 + a) + 1)`` (exact algebra; the literal form loses |x| / ulp bits near 0)."""
    _, ab, sqrt = _ops(x)
    x = _arr(x)
    return x / (sqrt(ab(x) + 1.0) + 1.0) + eps * x


def h_inv(y, eps: float = 1e-3):
    """``sign(y) (r^2 - 1)`` with ``r = (sqrt(1 + 4 eps (|y| + 1 + eps)) - 1) / (2 eps)``, evaluated as ``sign(y)
    t (t + 2)`` with ``t = r - 1 = 2 |y| / (sqrt(1 + 4 eps (|y| + 1 + eps)) + 1 + 2 eps)`` (exact algebra: ``1 + 4
    eps (|y| + 1 + eps) = (1 + 2 eps)^2 + 4 eps |y|``), which has no cancelling difference either."""
    sign, ab, sqrt = _ops(y)
    y = _arr(y)
    t = 2.0 * ab(y) / (sqrt(1.0 + 4.0 * eps * (ab(y) + 1.0 + eps)) + 1.0 + 2.0 * eps)
    return sign(y) * (t * (t + 2.0))


def rescale_target(R, Gamma, y, eps: float = 1e-3):
    """``T(R, Gamma, y) = h(R + Gamma h^-1(y))``, broadcasting its arguments."""
    return h(R + Gamma * h_inv(y, eps), eps)
