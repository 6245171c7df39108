"""Cost of the periodic shrink-and-perturb resets, ``Runtime.reset_interval``, three things:

(a) the isolated time of one reset at B = 512 in fp32 (split) and bf16 -- ``reset_perturb_kernel`` alone, and
    ``FusedNatureLearner.reset_now`` whole: the launch plus the repacks of the fused forward's fragment buffers
    and the reset word -- eager and back to back, timed with device events over ``--launches`` calls;
(b) the learner step rate of the fused NatureCNN learner (synthetic frames, the captured multi-update graphs)
    with ``reset_interval`` so large that no reset fires, against two default learners in the same process: the
    variants alternated ``--reps`` times so they see the same machine state.  A reset that never fires adds no
    launch, so the expectation is "inside the A/A spread of the two default learners";
(c) ``--vgpr`` (needs no GPU): the VGPR counts and scratch of the optimizer kernels' Adam instantiations, which
    read the reset word ``OptSched.t0``, from the compiler's resource report (scripts/check_spills.py).

Prints one JSON line (docs/PERF_NOTES.md "Periodic resets")."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEVER = 10 ** 9


def vgpr_report() -> dict:
    """{kernel: [VGPRs, scratch bytes]} of the step-indexed optimizer instantiations (MODE 2 = Adam)."""
    from check_spills import CSRC, usage
    out = {}
    for f in ("optimizer.hip", "sumtree.hip"):
        for r in usage(os.path.join(CSRC, f)):
            if any(k in r["name"] for k in ("opt_sched_kernel", "opt_ema_kernel", "rmsprop_sample_kernel")):
                out[r["name"]] = [r.get("VGPRs", 0), r.get("ScratchSize", 0)]
    return out


def timed_us(fn, launches: int) -> float:
    import torch
    for _ in range(3):
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
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--replay", type=int, default=100000)
    ap.add_argument("--vgpr", action="store_true", help="only the compiler's resource report (no GPU)")
    args = ap.parse_args()
    if args.vgpr:
        print(json.dumps({"metric": "vgprs_scratch", "kernels": vgpr_report()}), flush=True)
        return
    import torch

    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from bench_optimizer import make_replay
    if not torch.cuda.is_available():
        raise SystemExit("bench_reset.py needs a GPU (or --vgpr)")
    dev = torch.device("cuda", 0)
    learners = {}
    for dtype in ("fp32", "bf16"):
        for name, interval in (("default_a", 0), ("reset_never", NEVER), ("default_b", 0)):
            cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                        "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                        "Replay_Memory": {"soft_capacity": args.replay},
                                        "Runtime": {"dtype": dtype, "seed": 1234, "reset_interval": interval}})
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
    out = {"metric": "updates_per_s", "batch": args.batch, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), "params": int(learners["fp32_reset_never"].p32.numel())}
    for name, r in rates.items():
        L = learners[name]
        assert L.update_index() == L.num_q_updates and L.last_metrics().get("resets", 0) == 0
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r)}
    for dtype in ("fp32", "bf16"):
        a, b, x = (out[f"{dtype}_{k}"]["median"] for k in ("default_a", "default_b", "reset_never"))
        out[f"{dtype}_aa_spread"] = round(abs(a - b), 1)
        out[f"{dtype}_reset_never_vs_default_mean"] = round(x - 0.5 * (a + b), 1)
    # the isolated reset, last: it rewrites the learners' parameters
    for dtype in ("fp32", "bf16"):
        L = learners[f"{dtype}_reset_never"]
        kernel = lambda: L.ops.reset_perturb(L._reset_table, L._seed_r, 1, L.p32, L.t32, L.rms_v, L.rms_m,
                                             (L.pbf, L.pbf_lo), (L.tbf, L.tbf_lo))
        out[f"{dtype}_reset_kernel_us"] = timed_us(kernel, args.launches)
        out[f"{dtype}_reset_now_us"] = timed_us(lambda: L.reset_now(1), args.launches)
        planes = 2 if L.split else 1
        nbytes = int(L.p32.numel()) * (2 * 4 * 2 + 2 * 4 + 2 * 2 * planes)     # p, t read + written; v, m; the planes
        out[f"{dtype}_reset_kernel_gb_per_s"] = round(nbytes / out[f"{dtype}_reset_kernel_us"] * 1e-3, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
