"""Periodic shrink-and-perturb resets (Nikishin et al. 2022 "The Primacy Bias"; D'Oro et al. 2023, SR-SPR;
Schwarzer et al. 2023, BBF) of a learner that makes many updates per environment frame
(``Runtime.reset_interval`` = I): the host mirror of csrc/reset.hip and the definition.

After every update whose completed count ``num_q_updates`` is a positive multiple of I, reset
r = num_q_updates / I (numbered from 1) mixes every parameter with a fresh draw from its layer's initial
distribution, keeping the share alpha of the old value (``Runtime.reset_shrink_encoder`` for the conv layers,
``Runtime.reset_shrink_head`` for everything behind them), and zeroes the optimizer moments.  For flat
element index i of segment s:

  seed_r = mix64(Runtime.seed ^ "SPRreset") & (2^63 - 1)                   (:func:`reset_seed`)
  k      = apex_uniform(seed_r, r, i) 2^24                                 the 24-bit integer
  phi_i  = fp32((double)(2 k + 1 - 2^24) / 2^24 * (double)bound_s)         symmetric, never +-bound, rounded once
  p'_i   = fl(fl(alpha_s p_i) + fl(fl(1 - alpha_s) phi_i))                 fp32, no contraction
  t'_i   = the same expression on the target's t_i with the SAME phi_i
  v_i = m_i = 0                                                            whatever alpha

``bound_s = fp32(1 / sqrt(fan_in))`` is torch's default ``Linear`` / ``Conv2d`` range (a bias uses its weight's
fan-in).  A sigma segment of the noisy layers takes its initial constant sigma0 / sqrt(p) in the place of phi; the
zero-padded elements of ``nature32`` have phi = 0 and stay exact zeros; the alignment gaps between segments are
not touched.  Both nets mix in the same phi: a fully reset segment (alpha = 0) has target = online afterwards, a
shrunk one keeps its online - target gap scaled by alpha.  ``apex_uniform`` is the replay's counter RNG
(csrc/apex_common.h, replay/gpu_replay.py).
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence

import numpy as np

from ..replay.gpu_replay import _mix64

MAX_ROWS = 32       # csrc/reset.hip RESET_MAX_ROWS
ENCODER = ("w1", "b1", "w2", "b2", "w3", "b3")
_SIGMA_OF = {"swv": "wv", "sbv": "wv", "swa": "wa", "sba": "wa", "swfc": "wfc", "sbfc": "wfc"}
_WEIGHT_OF = {"b1": "w1", "b2": "w2", "b3": "w3", "bfc": "wfc", "bv": "wv", "ba": "wa", "btau": "wtau"}


class ResetRow(NamedTuple):
    """One segment of a reset: element i in [start, end) is drawn iff ``(i - start) % period < live`` (else
    phi = 0: the strided zero padding of ``nature32``); ``const_flag``: ``const_value`` in the place of phi."""
    start: int
    end: int
    period: int
    live: int
    bound: float
    alpha: float
    const_flag: int
    const_value: float


def reset_seed(seed: int) -> int:
    """seed_r of ``Runtime.seed``: mixed with its own constant, so the reset stream coincides with none of the
    replay's sampling stream, the noise stream, the tau stream and the shift stream."""
    with np.errstate(over="ignore"):
        return int(_mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64(0x5350527265736574))) & ((1 << 63) - 1)


def fan_in_bound(fan_in: int) -> np.float32:
    """fp32(1 / sqrt(fan_in)): torch's default ``Linear`` / ``Conv2d`` range."""
    return np.float32(1.0 / np.sqrt(np.float64(int(fan_in))))


def sigma_const(sigma0: float, p: int) -> np.float32:
    """What ``NoisyLinear`` fills a sigma tensor of fan-in ``p`` with (models/dueling.py)."""
    return np.float32(float(sigma0) / float(int(p)) ** 0.5)


def reset_table(layout, cfg) -> List[ResetRow]:
    """The rows of a ``FlatLayout`` (models/flat_params.py) under ``cfg``, in flat order: one per segment, the
    alignment gaps between them excluded."""
    rt = cfg.Runtime
    C = int(cfg.frame_stack)
    c1 = 32 if cfg.network == "nature32" else 64
    a_e, a_h = float(rt.reset_shrink_encoder), float(rt.reset_shrink_head)
    fan = {"w1": C * 64, "w2": 16 * c1, "w3": 576, "wfc": 3136, "wv": 512, "wa": 512, "wtau": 64}
    rows = []
    for name, shape in layout.segments:
        start = int(layout.offsets[name])
        n = int(np.prod(shape))
        period, live = n, n
        if name == "w1":                 # (64, C, 8, 8): the filters >= c1 are padding
            live = c1 * C * 64
        elif name in ("b1", "w2"):       # (64,), (64, 4, 4, 64): the channels >= c1 are padding
            period, live = 64, c1
        alpha = a_e if name in ENCODER else a_h
        if name in _SIGMA_OF:
            p = fan[_SIGMA_OF[name]]
            rows.append(ResetRow(start, start + n, period, live, float(fan_in_bound(p)), alpha, 1,
                                 float(sigma_const(rt.noisy_sigma0, p))))
        else:
            p = fan[_WEIGHT_OF.get(name, name)]
            rows.append(ResetRow(start, start + n, period, live, float(fan_in_bound(p)), alpha, 0, 0.0))
    check_table(rows, layout.numel, align=4)
    return rows


def module_reset_table(module, cfg) -> List[ResetRow]:
    """The rows of an ``nn.Module``'s parameters in ``named_parameters()`` order (the torch learner): flat index =
    running offset, fan-in from the shape (a bias and a sigma use their layer's weight), the ``layer*`` modules
    shrunk by ``reset_shrink_encoder`` and the rest by ``reset_shrink_head``."""
    rt = cfg.Runtime
    a_e, a_h = float(rt.reset_shrink_encoder), float(rt.reset_shrink_head)
    shapes = {k: tuple(p.shape) for k, p in module.named_parameters()}
    rows, off = [], 0
    for name, shape in shapes.items():
        n = int(np.prod(shape))
        stem, leaf = name.rsplit(".", 1)
        w = shapes[stem + ".weight"]
        p = int(np.prod(w[1:]))
        alpha = a_e if name.startswith("layer") else a_h
        sig = leaf.endswith("_sigma")
        rows.append(ResetRow(off, off + n, n, n, float(fan_in_bound(p)), alpha, int(sig),
                             float(sigma_const(rt.noisy_sigma0, p)) if sig else 0.0))
        off += n
    return rows


def check_table(table: Sequence[ResetRow], n: int, align: int = 1) -> None:
    """What the launcher checks (csrc/reset.hip ``reset_args_ok``, there with ``align`` = 4: a float4 chunk never
    straddles two rows): at most ``MAX_ROWS`` ordered, non-overlapping rows inside [0, n)."""
    if not 1 <= len(table) <= MAX_ROWS:
        raise ValueError(f"a reset table holds 1..{MAX_ROWS} rows, got {len(table)}")
    prev = 0
    for r in table:
        if r.start % align or not prev <= r.start < r.end <= n or not 0 <= r.live <= r.period or r.period < 1 \
                or not 0.0 <= r.alpha <= 1.0:
            raise ValueError(f"reset table row {tuple(r)} is unordered, misaligned or outside [0, {n})")
        prev = r.end


def u24(seed: int, ctr: int, idx) -> np.ndarray:
    """The 24-bit integer behind ``apex_uniform(seed, ctr, idx)`` (csrc/apex_common.h ``apex_u24``), uint64."""
    i = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        inner = _mix64(np.uint64(int(ctr) & 0xFFFFFFFFFFFFFFFF) * np.uint64(0x100000001B3) + i)
        return _mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ inner) >> np.uint64(40)


def row_values(seed_r: int, r: int, row: ResetRow) -> np.ndarray:
    """phi of one row's elements (fp32): the draw, the sigma constant, or 0 on the padding."""
    n = row.end - row.start
    if row.const_flag:
        return np.full(n, np.float32(row.const_value), dtype=np.float32)
    k = u24(seed_r, r, np.arange(row.start, row.end, dtype=np.uint64)).astype(np.int64)
    x = (2 * k + 1 - (1 << 24)).astype(np.float64) / np.float64(1 << 24)
    phi = (x * np.float64(np.float32(row.bound))).astype(np.float32)
    if row.live < row.period:
        phi[np.arange(n) % row.period >= row.live] = 0.0
    return phi


def fresh_values(seed_r: int, r: int, table: Sequence[ResetRow]) -> np.ndarray:
    """phi over [0, the last row's end) for reset ``r``: fp32, zeros in the gaps and on the padding."""
    out = np.zeros(int(table[-1].end), dtype=np.float32)
    for row in table:
        out[row.start:row.end] = row_values(seed_r, r, row)
    return out


def apply_reset(p, t, v, m, seed_r: int, r: int, table: Sequence[ResetRow]):
    """Reset ``r`` on the fp32 arrays ``p`` (online), ``t`` (target), ``v``, ``m`` (the moments), in place: bit for
    bit what ``reset_perturb_kernel`` computes.  Elements outside the table's rows are not touched."""
    for a in (p, t, v, m):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 1:
            raise TypeError("apply_reset mirrors fp32 arithmetic: pass flat float32 arrays")
    check_table(table, min(a.size for a in (p, t, v, m)))
    for row in table:
        s = slice(row.start, row.end)
        phi = row_values(seed_r, r, row)
        al = np.float32(row.alpha)
        be = np.float32(np.float32(1.0) - al)
        f = (be * phi).astype(np.float32)
        for a in (p, t):
            a[s] = ((al * a[s]).astype(np.float32) + f).astype(np.float32)
        v[s] = 0.0
        m[s] = 0.0
    return p, t, v, m
