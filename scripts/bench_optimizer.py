"""Learner step rate per update rule: ``learner.steps(200)`` of the fused NatureCNN
learner (B = 512, synthetic frames, the captured multi-update graphs) timed with device
events after a warm-up, for RMSprop (the default), Adam, and Adam with the lr and
IS-exponent schedules -- alternated ``--reps`` times in one process so the variants see
the same machine state.  bench.py measures the default only; this is the number for
``Runtime.optimizer = "adam"`` (same bytes as centered RMSprop: reads g, p, v, m, writes
p, v, m, hi, lo).  Prints one JSON line."""
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
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard  # noqa: E402

VARIANTS = {
    "rmsprop": {},
    "adam": {"optimizer": "adam"},
    "adam_sched": {"optimizer": "adam", "lr_warmup_steps": 100, "lr_decay_steps": 100000, "lr_end": 1e-5,
                   "is_beta_end": 1.0, "is_beta_anneal_steps": 100000},
}


def make_replay(cap: int, actions: int, dev) -> GpuReplayShard:
    frames_cap = cap + 4096
    rp = GpuReplayShard(cap, cap, frames_cap, 4, alpha=0.6, beta=0.4, device=dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(1000)
    rp.frames.copy_(torch.randint(0, 256, rp.frames.shape, generator=g, device=dev, dtype=torch.uint8))
    rp.frame_head = frames_cap
    rng = np.random.default_rng(0)
    for s in range(0, cap, 16384):
        K = min(16384, cap - s)
        st = rng.integers(0, frames_cap - 8, size=K)[:, None] + np.arange(4)[None]
        rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, actions, K), R=rng.normal(size=K).astype(np.float32),
                       Gamma=np.full(K, 0.99 ** 3, np.float32), priority=rng.random(K).astype(np.float32) + 0.01))
    rp.rebuild()
    return rp


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replay", type=int, default=100000)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer.py needs a GPU")
    dev = torch.device("cuda", 0)
    learners = {}
    for name, rt in VARIANTS.items():
        cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                    "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                    "Replay_Memory": {"soft_capacity": args.replay},
                                    "Runtime": {"dtype": args.dtype, "seed": 1234, **rt}})
        torch.manual_seed(0)
        L = FusedNatureLearner(cfg, dev, make_replay(args.replay, 6, dev))
        L.prepare_graphs(multi=True)
        L.steps(args.warmup)
        torch.cuda.synchronize()
        learners[name] = L
    rates = {name: [] for name in VARIANTS}
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
           "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r)}
        L = learners[name]
        out[name]["update_index"] = L.update_index()
        assert L.update_index() == L.num_q_updates
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
