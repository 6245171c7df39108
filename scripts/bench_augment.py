"""Cost of the random-shift augmentation, ``Runtime.augment_shift``, three numbers from one process:

(a) the isolated time of ``augment_shift_kernel`` at B = 512, C = 4, P = 4 (2B C = 4096 frames gathered
    from the replay ring by sampled slots, 28.9 MB read and 28.9 MB written), eager and back to back, timed
    with device events over ``--launches`` calls;
(b) the time of a device-to-device ``copy_`` of a 28.9 MB buffer, the same 2 x 28.9 MB of traffic with no
    gather and no LDS work: the yardstick;
(c) the learner step rate of the fused NatureCNN learner (synthetic frames, the captured multi-update
    graphs) at P = 0 and P = 4, in fp32 (split) and bf16, the variants alternated ``--reps`` times so they
    see the same machine state.

Prints one JSON line (docs/PERF_NOTES.md "Random-shift augmentation")."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apex_dqn_amd.config import ApexConfig  # noqa: E402
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner  # noqa: E402
from bench_optimizer import make_replay  # noqa: E402

PAD = 4


def timed_us(fn, launches: int) -> float:
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / launches, 2)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--replay", type=int, default=100000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py needs a GPU")
    dev = torch.device("cuda", 0)
    learners = {}
    for dtype in ("fp32", "bf16"):
        for name, pad in (("off", 0), ("shift", PAD)):
            cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                        "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                        "Replay_Memory": {"soft_capacity": args.replay},
                                        "Runtime": {"dtype": dtype, "seed": 1234, "augment_shift": pad}})
            torch.manual_seed(0)
            L = FusedNatureLearner(cfg, dev, make_replay(args.replay, 6, dev))
            L.prepare_graphs(multi=True)
            L.steps(args.warmup)
            torch.cuda.synchronize()
            learners[f"{dtype}_{name}"] = L
    rates = {name: [] for name in learners}
    for _ in range(args.reps):
        for name, L in learners.items():
            caps = L.graph_captures
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.steps(args.steps)
            e1.record()
            torch.cuda.synchronize()
            assert L.graph_captures == caps, "a graph capture landed in the timed window"
            rates[name].append(round(args.steps / (e0.elapsed_time(e1) * 1e-3), 1))
    L = learners["fp32_shift"]
    nbytes = int(L.aug_frames.numel())
    src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    kernel_us = timed_us(L._augment_step, args.launches)
    copy_us = timed_us(lambda: dst.copy_(src), args.launches)
    out = {"metric": "updates_per_s", "batch": args.batch, "steps": args.steps, "pad": PAD,
           "device": torch.cuda.get_device_name(0), "frames": int(L.aug_frames.shape[0]), "bytes_each_way": nbytes,
           "augment_kernel_us": kernel_us, "d2d_copy_us": copy_us, "kernel_over_copy": round(kernel_us / copy_us, 3),
           "kernel_gb_per_s": round(2 * nbytes / kernel_us * 1e-3, 1),
           "augment_offset_mean": L.last_metrics()["augment_offset_mean"]}
    for name, r in rates.items():
        assert learners[name].update_index() == learners[name].num_q_updates
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r),
                     "us_per_update": round(1e6 / float(np.median(r)), 2)}
    for dtype in ("fp32", "bf16"):
        out[f"{dtype}_delta_us_per_update"] = round(out[f"{dtype}_shift"]["us_per_update"]
                                                    - out[f"{dtype}_off"]["us_per_update"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
