"""Learner step rate of the quantile-regression (QR-DQN) head against the scalar and the
categorical (C51) head, by the protocol of ``scripts/bench_c51.py``: ``learner.steps(200)`` of
the fused NatureCNN learner (B = 512, synthetic frames, the captured multi-update graphs)
timed with device events after a warm-up.  Per action count four learners -- scalar, C51 with
``--atoms`` atoms, quantile with ``--atoms`` and with each of ``--quantiles`` quantiles -- alternated
``--reps`` times in one process so they see the same machine state; every ratio is against
the scalar-head number of the same run.  ``--dtype`` fp32 (split) or bf16.  Prints one JSON
line."""
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replay", type=int, default=100000)
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("--quantiles", type=int, nargs="+", default=[32])     # e.g. 32 200: above 64, csrc/qr_wide_head.hip
    ap.add_argument("--out", default="")       # also write the JSON line to this file
    ap.add_argument("--actions", type=int, nargs="+", default=[4, 18])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qr.py needs a GPU")
    dev = torch.device("cuda", 0)
    heads = {"scalar": {"num_atoms": 1},
             f"c51_{args.atoms}": {"num_atoms": args.atoms},
             f"qr_{args.atoms}": {"num_atoms": args.atoms, "dist_head": "quantile"},
             **{f"qr_{n}": {"num_atoms": n, "dist_head": "quantile"} for n in args.quantiles}}
    learners = {}
    for A in args.actions:
        for name, head in heads.items():
            cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                        "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                        "Replay_Memory": {"soft_capacity": args.replay},
                                        "Runtime": {"dtype": args.dtype, "seed": 1234, **head}})
            torch.manual_seed(0)
            L = FusedNatureLearner(cfg, dev, make_replay(args.replay, A, dev))
            L.prepare_graphs(multi=True)
            L.steps(args.warmup)
            torch.cuda.synchronize()
            learners[f"A{A}_{name}"] = L
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
    out = {"metric": "updates_per_s", "batch": args.batch, "steps": args.steps, "dtype": args.dtype,
           "atoms": args.atoms, "quantiles": args.quantiles, "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r)}
        assert np.isfinite(learners[name].last_metrics()["loss"])
    for A in args.actions:
        s = out[f"A{A}_scalar"]["median"]
        for name in heads:
            if name != "scalar":
                c = out[f"A{A}_{name}"]["median"]
                out[f"A{A}_{name}_vs_scalar"] = round(c / s, 4)
                out[f"A{A}_{name}_extra_us_per_update"] = round(1e6 / c - 1e6 / s, 1)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
