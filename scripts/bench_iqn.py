"""Isolated times of the implicit quantile (IQN) head kernels (csrc/iqn_head.hip) at the learner's
batch, beside the quantile-regression head's launches at the same (A, N) in the same process:

  iqn_head     ``iqn_head_kernel``   against   qr_head     ``qr_head_kernel``
  iqn_wgrad    ``iqn_wgrad_prio_kernel`` (no priority block)  against   head_wgrad  the wide head weight gradient

Each launch is timed with device events over ``--iters`` back-to-back launches after a warm-up,
the four alternated ``--reps`` times so they see the same machine state.  Inputs are random with
the statistics of tests/iqn_fixtures.py; ``--dtype`` fp32 (split hi / lo activation planes) or
bf16.  ``--steps-mode``: instead, the learner step rate by the protocol of ``scripts/bench_qr.py``
(``learner.steps(200)`` of the fused NatureCNN learner at B = 512, captured multi-update graphs,
device events after a warm-up): per action count the scalar head, and per sample count N the
quantile head and the implicit head, alternated ``--reps`` times in one process; every ratio is
against the quantile head at the same N.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apex_dqn_amd.ops.fused_ops import HipBackend  # noqa: E402


def problem(B, A, N, split, dev):
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g)                          # noqa: E731

    def planes(x):
        hi = x.to(torch.bfloat16)
        return hi.to(dev), ((x - hi.float()).to(torch.bfloat16).to(dev) if split else None)
    (Hon, Hon_lo), (Htg, Htg_lo) = planes(torch.relu(r(2 * B, 1024))), planes(torch.relu(r(B, 1024)))
    head = lambda n: {"wv": (r(n, 512) * 0.05).to(dev), "bv": r(n).to(dev),      # noqa: E731
                      "wa": (r(A * n, 512) * 0.05).to(dev), "ba": r(A * n).to(dev)}
    emb = lambda: {"wtau": (r(1024, 64) * 0.125).to(dev), "btau": (r(1024) * 0.1 ** 0.5).to(dev)}    # noqa: E731
    return dict(Hon=Hon, Htg=Htg, lo=(Hon_lo, Htg_lo), P1=(head(1), head(1)), PN=(head(N), head(N)), E=(emb(), emb()),
                act=torch.randint(0, A, (B,), generator=g).to(torch.int32).to(dev), rew=(r(B) * 3).to(dev),
                gam=torch.full((B,), 0.97, device=dev), isw=torch.rand(B, generator=g).to(dev))


def steps_main(args) -> None:
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from bench_optimizer import make_replay
    dev = torch.device("cuda", 0)
    heads = {"scalar": {"num_atoms": 1}}
    for N in args.samples:
        heads[f"qr_{N}"] = {"num_atoms": N, "dist_head": "quantile"}
        heads[f"iqn_{N}"] = {"num_atoms": N, "dist_head": "implicit"}
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
           "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r)}
        assert np.isfinite(learners[name].last_metrics()["loss"])
    for A in args.actions:
        for N in args.samples:
            q, i = out[f"A{A}_qr_{N}"]["median"], out[f"A{A}_iqn_{N}"]["median"]
            out[f"A{A}_iqn_{N}_vs_qr"] = round(i / q, 4)
            out[f"A{A}_iqn_{N}_extra_us_per_update"] = round(1e6 / i - 1e6 / q, 1)
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-mode", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--replay", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--actions", type=int, nargs="+", default=[4, 18])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iqn.py needs a GPU")
    if args.steps_mode:
        return steps_main(args)
    dev = torch.device("cuda", 0)
    be = HipBackend()
    split, B = args.dtype == "fp32", args.batch
    out = {"metric": "us_per_launch", "batch": B, "iters": args.iters, "dtype": args.dtype,
           "device": torch.cuda.get_device_name(0)}
    for A in args.actions:
        for N in args.samples:
            p = problem(B, A, N, split, dev)
            z = lambda *s: torch.zeros(*s, device=dev)                    # noqa: E731
            td, loss, dhead = z(B), z(B), z(B, (A + 1) * N)
            dH = torch.zeros(B, 1024, device=dev, dtype=torch.bfloat16)
            lo = (p["lo"][0], p["lo"][1], torch.zeros_like(dH)) if split else None
            ws = be.iqn_workspace(B, N, dev)
            gi = {"wv": z(1, 512), "bv": z(1), "wa": z(A, 512), "ba": z(A), "wtau": z(1024, 64), "btau": z(1024)}
            gq = {"wv": z(N, 512), "bv": z(N), "wa": z(A * N, 512), "ba": z(A * N)}
            ctr = torch.zeros(1, dtype=torch.int64, device=dev)
            launches = {
                "iqn_head": lambda: be.iqn_head(p["Hon"], p["Htg"], *p["P1"], *p["E"], p["act"], p["rew"], p["gam"],
                                                p["isw"], N, 1.0, 1.0 / B, 99, ctr, None, td, loss, dH, dhead, ws, lo=lo),
                "iqn_wgrad": lambda: be.iqn_wgrad(p["act"], ws, gi),
                "qr_head": lambda: be.qr_head(p["Hon"], p["Htg"], *p["PN"], p["act"], p["rew"], p["gam"], p["isw"], N, 1.0,
                                              1.0 / B, td, loss, dH, dhead, lo=lo),
                "head_wgrad": lambda: be.head_wgrad(p["Hon"], dhead, gq, Hon_lo=p["lo"][0]),
            }
            times = {k: [] for k in launches}
            for fn in launches.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for name, fn in launches.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(round(e0.elapsed_time(e1) * 1e3 / args.iters, 2))
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(gi["wtau"]).all())
            # what the algorithm needs: 3 N embeddings + 3 N head rows forward, the set-0 backward, the wtau product
            flop = B * N * (3 * 2 * 1024 * 64 + 3 * 2 * 1024 * (A + 1) / 2 + 2 * 1024 * 64 + 2 * 1024 * 64)
            row = {k: {"runs": v, "median": float(np.median(v))} for k, v in times.items()}
            row["iqn_total_us"] = round(row["iqn_head"]["median"] + row["iqn_wgrad"]["median"], 2)
            row["qr_total_us"] = round(row["qr_head"]["median"] + row["head_wgrad"]["median"], 2)
            row["iqn_gflop"] = round(flop * 1e-9, 3)
            row["dpre_mbytes"] = round(B * N * 1024 * 4 / 2 ** 20, 1)
            out[f"A{A}_N{N}"] = row
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
