"""Learner step rate with the Munchausen-DQN target (``Runtime.munchausen``) off and on, by the
protocol of ``scripts/bench_noisy.py``: ``learner.steps(200)`` of the fused NatureCNN learner
(B = 512, synthetic frames, the captured multi-update graphs) timed with device events after a
warm-up.  The two learners are alternated ``--reps`` times in one process so they see the same
machine state; the ratio is against the default (n-step double DQN) learner of the same run.
Then the isolated times of the two head kernels on the learners' own buffers (csrc/ddqn_head.hip
reading h, i.e. without the deferred fc epilogue it carries in the default step, and
csrc/mdqn_head.hip), ``--kernel-iters`` back-to-back launches between two device events.
``--dtype`` fp32 (split) or bf16.  Prints one JSON line."""
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
from bench_noisy import kernel_us  # noqa: E402
from bench_optimizer import make_replay  # noqa: E402


def head_launch(L):
    """The learner's head launch alone, on its own buffers (h as the last forward left it)."""
    B, rt, S, sp = L.B, L.rt, L.S, L.split
    isw = S["weights"] if L._isw else None
    args = (L._head_params(L.P), L._head_params(L.T), S["act"], S["rew"], S["gam"], isw, rt.loss == "huber",
            rt.huber_delta)
    tail = (1.0 / B, L.td_abs, L.loss_b, L.dH, L.dhead)
    if L.munchausen:
        mk = L.cfg.munchausen_kw()
        lo = dict(lo=(L.h_lo[:B], L.h_lo[B:], L.dH_lo)) if sp else {}
        return lambda: L.ops.mdqn_head(L.h[:B], L.h[B:], *args, mk["alpha"], mk["tau"], mk["clip"], *tail,
                                       aux=L.mdqn_aux, zero=L.g_head_region, isn=L._isn(), **lo)
    lo = dict(lo=(L.h_lo[:2 * B], L.h_lo[2 * B:], L.dH_lo)) if sp else {}
    return lambda: L.ops.head(L.h[:2 * B], L.h[2 * B:], *args, *tail, zero=L.g_head_region, isn=L._isn(), **lo)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replay", type=int, default=100000)
    ap.add_argument("--actions", type=int, default=4)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_munchausen.py needs a GPU")
    dev = torch.device("cuda", 0)
    A = args.actions
    learners = {}
    for name, on in (("default", False), ("munchausen", True)):
        cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                    "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                    "Replay_Memory": {"soft_capacity": args.replay},
                                    "Runtime": {"dtype": args.dtype, "seed": 1234, "munchausen": on}})
        torch.manual_seed(0)
        L = FusedNatureLearner(cfg, dev, make_replay(args.replay, A, dev))
        L.prepare_graphs(multi=True)
        L.steps(args.warmup)
        torch.cuda.synchronize()
        learners[name] = L
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
    out = {"metric": "updates_per_s", "batch": args.batch, "steps": args.steps, "dtype": args.dtype, "actions": A,
           "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r)}
        assert np.isfinite(learners[name].last_metrics()["loss"])
    d, m = out["default"]["median"], out["munchausen"]["median"]
    out["munchausen_vs_default"] = round(m / d, 4)
    out["munchausen_extra_us_per_update"] = round(1e6 / m - 1e6 / d, 1)
    out["ddqn_head_us"] = kernel_us(head_launch(learners["default"]), args.kernel_iters)
    out["mdqn_head_us"] = kernel_us(head_launch(learners["munchausen"]), args.kernel_iters)
    mm = learners["munchausen"].last_metrics()
    out["munchausen_bonus_mean"], out["soft_value_mean"] = mm["munchausen_bonus_mean"], mm["soft_value_mean"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
