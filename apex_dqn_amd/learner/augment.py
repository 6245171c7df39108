"""Random-shift frame augmentation (DrQ, Kostrikov et al. 2020; DrQ(eps), Agarwal et al. 2021)
of the sampled batch (``Runtime.augment_shift`` = P): the host mirror of csrc/augment.hip and
the definition.  Integer arithmetic only, so the kernel, the torch backend's oracle and the
torch learner agree byte for byte.

Every sampled state is padded by P pixels with edge replication and cropped back to 84 x 84 at
an offset (o_y, o_x) in [0, 2P]^2.  For update index u (the updates completed, as the noisy
compose reads it) and batch row r in [0, 2B) -- rows [0, B) are S_t, rows [B, 2B) S_t+n:

  seed_a  = mix64(Runtime.seed ^ "DrQshift") & (2^63 - 1)            (:func:`aug_seed`)
  k(axis) = apex_uniform(seed_a, 64 u, 2 r + axis) 2^24              the 24-bit integer; axis 0 = y, 1 = x
  o(axis) = (k (2P + 1)) >> 24
  out[r][c][y][x] = in[r][c][clamp(y + o_y - P, 0, 83)][clamp(x + o_x - P, 0, 83)]

One shift per (sample, state): the C frames of a stack share it, and so does every forward row
that shows that state -- the third row block of the step (the target net at S_t+n, or at S_t
with the Munchausen target) reads the augmented copy of the rows it repeats
(:func:`aug_slot_table`).  ``apex_uniform`` is the replay's counter RNG (csrc/apex_common.h,
replay/gpu_replay.py).
"""
from __future__ import annotations

import numpy as np
import torch

from ..replay.gpu_replay import _mix64, apex_uniform
from .noisy import STREAMS_PER_INDEX

MAX_PAD = 8
HW = 84


def aug_seed(seed: int) -> int:
    """seed_a of ``Runtime.seed``: mixed with its own constant, so the shift stream coincides with
    none of the replay's sampling stream, the noise stream and the tau stream."""
    with np.errstate(over="ignore"):
        return int(_mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64(0x4472517368696674))) & ((1 << 63) - 1)


def check_pad(P: int) -> int:
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or not 1 <= int(P) <= MAX_PAD:
        raise ValueError(f"the shift's pad must be an integer in [1, {MAX_PAD}], got {P!r}")
    return int(P)


def shift_offsets(seed_a: int, u: int, rows: int, P: int) -> torch.Tensor:
    """int32 [rows, 2]: (o_y, o_x) in [0, 2P] of every batch row at update ``u`` (``seed_a``:
    :func:`aug_seed`)."""
    P = check_pad(P)
    idx = np.arange(2 * int(rows), dtype=np.uint64)
    k = (apex_uniform(seed_a, STREAMS_PER_INDEX * int(u), idx).astype(np.float64) * 16777216.0).astype(np.uint64)
    o = (k * np.uint64(2 * P + 1)) >> np.uint64(24)
    return torch.from_numpy(o.astype(np.int32).reshape(int(rows), 2))


def shift_frames(frames_u8: torch.Tensor, offsets: torch.Tensor, P: int) -> torch.Tensor:
    """``frames_u8`` [rows, C, 84, 84] (natural pixel order) shifted row by row by ``offsets``
    [rows, 2]: index arithmetic with clamped coordinates, no padded copy."""
    P = check_pad(P)
    rows, _, H, W = frames_u8.shape
    assert (H, W) == (HW, HW) and tuple(offsets.shape) == (rows, 2)
    off = offsets.to(device=frames_u8.device, dtype=torch.long)
    ar = torch.arange(HW, device=frames_u8.device)
    sy = (ar[None, :] + off[:, 0:1] - P).clamp_(0, HW - 1)      # [rows, 84]
    sx = (ar[None, :] + off[:, 1:2] - P).clamp_(0, HW - 1)
    r = torch.arange(rows, device=frames_u8.device)
    return frames_u8[r[:, None, None], :, sy[:, :, None], sx[:, None, :]].permute(0, 3, 1, 2).contiguous()


def aug_slot_table(B: int, C: int, munchausen: bool = False) -> torch.Tensor:
    """int32 [3B, C]: the step's static slot table into the augmented buffer of 2B C frames.  Row
    r < 2B, frame c -> r C + c; the third row block repeats the rows of S_t+n (the default plan:
    the target net at S_t+n) or of S_t (the Munchausen plan: the target net at S_t)."""
    B, C = int(B), int(C)
    t = torch.arange(2 * B * C, dtype=torch.int32).reshape(2 * B, C)
    return torch.cat([t, t[:B] if munchausen else t[B:]]).contiguous()
