"""Cost of the rescaled n-step target, ``Runtime.value_rescale``: the learner step rate of the fused
NatureCNN learner (B = 512, synthetic frames, the captured multi-update graphs) with the key off and on, for
the scalar head and the 64-quantile head, in fp32 (split) and bf16, the variants alternated ``--reps`` times
in one process so they see the same machine state; and the isolated time of the head launch both ways (the
launch of the step, eager, timed with device events over ``--launches`` calls).  The key adds two fp64 square
roots and two fp64 divisions per target value: 512 values on the scalar head, 32 k on the quantile head
(docs/PERF_NOTES.md "Value rescaling").  ``--heads scalar`` runs the scalar head alone (the default path
against another checkout of the tree: run the same command in both, alternated).  Prints one JSON line."""
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

HEADS = {"scalar": {}, "quantile": {"num_atoms": 64, "dist_head": "quantile"}}


def isolated_head_us(L: FusedNatureLearner, launches: int) -> float:
    """Mean time of the learner's own head launch on the activations its last step left, eager and back to back
    (the scalar head then reads h: the deferred fc epilogue belongs to the step, not to this figure)."""
    isw = L.S["weights"] if L.rt.use_is_weights else None
    torch.cuda.synchronize()
    for _ in range(10):
        L._loss_head(isw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        L._loss_head(isw)
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
    ap.add_argument("--heads", default="scalar,quantile")
    ap.add_argument("--off-only", action="store_true", help="the key off only (a tree without the key runs this too)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_value_rescale.py needs a GPU")
    dev = torch.device("cuda", 0)
    learners = {}
    for head in args.heads.split(","):
        for dtype in ("fp32", "bf16"):
            for name in ("off",) if args.off_only else ("off", "on"):
                rt = {"dtype": dtype, "seed": 1234, **HEADS[head]}
                if name == "on":
                    rt["value_rescale"] = True
                cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                            "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                            "Replay_Memory": {"soft_capacity": args.replay}, "Runtime": rt})
                torch.manual_seed(0)
                L = FusedNatureLearner(cfg, dev, make_replay(args.replay, 6, dev))
                L.prepare_graphs(multi=True)
                L.steps(args.warmup)
                torch.cuda.synchronize()
                learners[f"{head}_{dtype}_{name}"] = L
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
    out = {"metric": "updates_per_s", "batch": args.batch, "steps": args.steps,
           "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        L = learners[name]
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r),
                     "us_per_update": round(1e6 / float(np.median(r)), 2),
                     "head_launch_us": isolated_head_us(L, args.launches)}
    if not args.off_only:
        for head in args.heads.split(","):
            for dtype in ("fp32", "bf16"):
                a, b = out[f"{head}_{dtype}_off"], out[f"{head}_{dtype}_on"]
                out[f"{head}_{dtype}_delta_us_per_update"] = round(b["us_per_update"] - a["us_per_update"], 2)
                out[f"{head}_{dtype}_delta_head_us"] = round(b["head_launch_us"] - a["head_launch_us"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
