"""Learner step rate of the histogram-loss (HL-Gauss) target against the categorical (C51) head it shares its
weights with, by the protocol of ``scripts/bench_qr.py``: ``learner.steps(200)`` of the fused NatureCNN learner
(B = 512, synthetic frames, the captured multi-update graphs) timed with device events after a warm-up.  Per
action count three learners -- C51 twice (``c51_a`` / ``c51_b``: the A/A spread of two learners of one config)
and HL-Gauss, all with ``--atoms`` atoms -- alternated ``--reps`` times in one process so they see the same
machine state.  Then the loss-head launch alone (``hlg_head_kernel`` against ``c51_head_kernel``) on each
learner's own buffers, ``--kernel-iters`` eager launches between two device events.  ``--dtype`` fp32 (split)
or bf16.  Prints one JSON line."""
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


def head_us(L, iters: int) -> float:
    """Microseconds per loss-head launch of learner ``L`` on the activations its last step left."""
    isw = L.S["weights"] if L._isw else None
    for _ in range(10):
        L._loss_head(isw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        L._loss_head(isw)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / iters, 2)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replay", type=int, default=100000)
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("--sigma-ratio", type=float, default=0.75)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--actions", type=int, nargs="+", default=[4, 18])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hlgauss.py needs a GPU")
    dev = torch.device("cuda", 0)
    c51 = {"num_atoms": args.atoms}
    heads = {"c51_a": c51, "c51_b": c51,
             "hlgauss": {"num_atoms": args.atoms, "dist_head": "hl_gauss", "hl_gauss_sigma_ratio": args.sigma_ratio}}
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
           "atoms": args.atoms, "sigma_ratio": args.sigma_ratio, "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r)}
        assert np.isfinite(learners[name].last_metrics()["loss"])
    for A in args.actions:
        a, b, h = (out[f"A{A}_{n}"]["median"] for n in ("c51_a", "c51_b", "hlgauss"))
        ref = 0.5 * (a + b)
        out[f"A{A}_aa_spread"] = round(abs(a - b) / ref, 4)
        out[f"A{A}_hlgauss_vs_c51"] = round(h / ref, 4)
        out[f"A{A}_hlgauss_extra_us_per_update"] = round(1e6 / h - 1e6 / ref, 1)
        out[f"A{A}_head_us"] = {"c51_head_kernel": head_us(learners[f"A{A}_c51_a"], args.kernel_iters),
                                "hlg_head_kernel": head_us(learners[f"A{A}_hlgauss"], args.kernel_iters)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
