"""Cost of the soft (Polyak) target, ``Runtime.target_ema_rate``: the learner step rate of the
fused NatureCNN learner (B = 512, synthetic frames, the captured multi-update graphs) at
rho = 0 (the hard sync of every 2500 updates) and rho = 0.005, in fp32 (split) and bf16, the
variants alternated ``--reps`` times in one process so they see the same machine state; and
the isolated time of the optimizer + sample launch both ways at the step's parameter count
(the launch of the step, eager, timed with device events over ``--launches`` calls).  The
EMA launch reads and writes t32 and writes the target's bf16 planes on top of the optimizer's
own traffic (docs/PERF_NOTES.md "Polyak target").  Prints one JSON line."""
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

RHO = 0.005


def isolated_launch_us(L: FusedNatureLearner, launches: int) -> float:
    """Mean time of the learner's own optimizer (+ sample, + fragment stores) launch, eager and back to
    back; the learner's state is restored afterwards."""
    snap = L._snapshot()
    torch.cuda.synchronize()
    for _ in range(10):
        L._seg3()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        L._seg3()
    e1.record()
    torch.cuda.synchronize()
    L._restore(snap)
    if L._presample:
        L._sample()
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
        raise SystemExit("bench_target_ema.py needs a GPU")
    dev = torch.device("cuda", 0)
    learners = {}
    for dtype in ("fp32", "bf16"):
        for name, rho in (("hard", 0.0), ("ema", RHO)):
            cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                        "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                        "Replay_Memory": {"soft_capacity": args.replay},
                                        "Runtime": {"dtype": dtype, "seed": 1234, "target_ema_rate": rho}})
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
    out = {"metric": "updates_per_s", "batch": args.batch, "steps": args.steps, "rho": RHO,
           "params": int(next(iter(learners.values())).p32.numel()), "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        L = learners[name]
        assert L.update_index() == L.num_q_updates
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r),
                     "us_per_update": round(1e6 / float(np.median(r)), 2),
                     "optimizer_launch_us": isolated_launch_us(L, args.launches),
                     "target_frags_in_launch": L._frag_out_t is not None}
    for dtype in ("fp32", "bf16"):
        h, e = out[f"{dtype}_hard"], out[f"{dtype}_ema"]
        out[f"{dtype}_delta_us_per_update"] = round(e["us_per_update"] - h["us_per_update"], 2)
        out[f"{dtype}_delta_launch_us"] = round(e["optimizer_launch_us"] - h["optimizer_launch_us"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
