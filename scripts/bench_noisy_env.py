"""One captured actor inference call with ``Runtime.noisy_actor_noise`` "shared" against "per_env" (csrc/noisy_actor.hip),
at E = 128 and 256 envs in both actor precisions, on the same GPU in one process.  Per (E, precision) two
``GpuActorGroup`` s over one fp32 learner (the rainbow config's head: C51 with ``--atoms`` atoms) capture their
inference as a HIP graph; after a warm-up the two graphs are replayed ``--iters`` times back to back between two device
events, alternated ``--reps`` times so both see the same machine state, and the median per call is reported.  Nothing
else runs on the GPU (no learner step beside the actors).  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apex_dqn_amd.actors.gpu_actor import GpuActorGroup  # noqa: E402
from apex_dqn_amd.config import ApexConfig  # noqa: E402
from apex_dqn_amd.envs.vector_envs import make_vec_env  # noqa: E402
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner  # noqa: E402
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard  # noqa: E402


def group(mode: str, E: int, precision: str, atoms: int, A: int, dev):
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Actor": {"num_actors": E, "epsilon": 0.0}, "Learner": {"replay_sample_size": 32},
                                "Runtime": {"use_graphs": False, "dtype": "fp32", "noisy": True, "num_atoms": atoms,
                                            "noisy_actor_noise": mode, "actor_precision": precision,
                                            "actor_graph": True}})
    torch.manual_seed(0)
    rp = GpuReplayShard(2000, 2000, 2400, 4, device=dev)
    L = FusedNatureLearner(cfg, dev, rp)
    g = GpuActorGroup(cfg, L, rp, make_vec_env(cfg.env_backend, cfg.env_conf.name, E, A, seed=0), E)
    seqs = rp.append_frames(np.random.default_rng(0).integers(0, 255, (E + 8, 84, 84), dtype=np.uint8))
    g.policy(np.stack([seqs[i:i + 4] for i in range(E)]))      # slots in, the graph captured
    assert g._graph is not None and g.env_noise == (mode == "per_env")
    return g


def replay_us(g, iters: int) -> float:
    with torch.cuda.stream(g.stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            g._graph.replay()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("--actions", type=int, default=6)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noisy_env.py needs a GPU")
    dev = torch.device("cuda", 0)
    out = {"metric": "us_per_captured_actor_call", "atoms": args.atoms, "actions": args.actions, "iters": args.iters,
           "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for E in args.envs:
        for precision in ("learner", "bf16"):
            gs = {m: group(m, E, precision, args.atoms, args.actions, dev) for m in ("shared", "per_env")}
            for g in gs.values():
                replay_us(g, args.warmup)
            runs = {m: [] for m in gs}
            for _ in range(args.reps):
                for m, g in gs.items():
                    runs[m].append(round(replay_us(g, args.iters), 2))
            key = f"E{E}_{'fp32' if precision == 'learner' else 'bf16'}"
            med = {m: float(np.median(r)) for m, r in runs.items()}
            out[key] = {"shared": {"runs": runs["shared"], "median": med["shared"]},
                        "per_env": {"runs": runs["per_env"], "median": med["per_env"]},
                        "per_env_minus_shared_us": round(med["per_env"] - med["shared"], 2),
                        "per_env_vs_shared": round(med["per_env"] / med["shared"], 4)}
            assert all(bool(torch.isfinite(g.q).all()) for g in gs.values())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
