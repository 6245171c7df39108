"""Learner step rate with the factorised NoisyNet fc and head layers (``Runtime.noisy``) off
and on, by the protocol of ``scripts/bench_qr.py``: ``learner.steps(200)`` of the fused
NatureCNN learner (B = 512, synthetic frames, the captured multi-update graphs) timed with
device events after a warm-up.  Four learners -- the scalar head and C51 with ``--atoms``
atoms, each without and with noisy layers -- alternated ``--reps`` times in one process so
they see the same machine state; every ratio is against the non-noisy learner of the same
head in the same run.  Then the isolated times of the two new kernels (csrc/noisy.hip:
the compose launch for both nets, the sigma-gradient launch) on the noisy learners' own
buffers, ``--kernel-iters`` back-to-back launches between two device events.  ``--dtype``
fp32 (split) or bf16.  Prints one JSON line."""
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


def kernel_us(fn, iters: int) -> float:
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
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
    ap.add_argument("--actions", type=int, default=6)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noisy.py needs a GPU")
    dev = torch.device("cuda", 0)
    heads = {"scalar": {"num_atoms": 1}, f"c51_{args.atoms}": {"num_atoms": args.atoms}}
    A = args.actions
    learners = {}
    for name, head in heads.items():
        for noisy in (False, True):
            cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                        "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                        "Replay_Memory": {"soft_capacity": args.replay},
                                        "Runtime": {"dtype": args.dtype, "seed": 1234, "noisy": noisy, **head}})
            torch.manual_seed(0)
            L = FusedNatureLearner(cfg, dev, make_replay(args.replay, A, dev))
            L.prepare_graphs(multi=True)
            L.steps(args.warmup)
            torch.cuda.synchronize()
            learners[f"{name}_{'noisy' if noisy else 'plain'}"] = L
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
           "atoms": args.atoms, "actions": A, "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r)}
        assert np.isfinite(learners[name].last_metrics()["loss"])
    for name in heads:
        p, n = out[f"{name}_plain"]["median"], out[f"{name}_noisy"]["median"]
        out[f"{name}_noisy_vs_plain"] = round(n / p, 4)
        out[f"{name}_noisy_extra_us_per_update"] = round(1e6 / n - 1e6 / p, 1)
        L = learners[f"{name}_noisy"]
        out[f"{name}_compose_2nets_us"] = kernel_us(L._noisy_compose, args.kernel_iters)
        out[f"{name}_sigma_grad_us"] = kernel_us(L._noisy_sigma_grad, args.kernel_iters)
        out[f"{name}_noisy_sigma_mean"] = L.last_metrics()["noisy_sigma_mean"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
