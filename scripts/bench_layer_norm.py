"""Cost of ``Runtime.layer_norm`` (LayerNorm on the two stream layers, csrc/fc_layernorm.hip), three things:

(a) the learner step rate of the fused NatureCNN learner (synthetic frames, the captured multi-update graphs) with
    the flag on against two default learners in the same process, fp32 (split) and bf16 at ``--batch`` rows: the
    variants alternated ``--reps`` times so they see the same machine state; the two default learners give the
    A/A spread the difference is read against;
(b) the isolated times of the three kernels' launches, eager and back to back, timed with device events over
    ``--launches`` calls: the LayerNorm epilogue against the plain epilogue (each behind its GEMM: fc_fwd whole),
    and the backward with its reduce;
(c) ``--vgpr`` (needs no GPU): VGPRs and scratch of the three kernels from the compiler's resource report
    (scripts/check_spills.py).

Prints one JSON line (docs/PERF_NOTES.md "Layer norm")."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vgpr_report() -> dict:
    """{kernel: [VGPRs, scratch bytes]} of csrc/fc_layernorm.hip."""
    from check_spills import CSRC, usage
    return {r["name"]: [r.get("VGPRs", 0), r.get("ScratchSize", 0)] for r in usage(os.path.join(CSRC, "fc_layernorm.hip"))}


def main() -> None:
    from bench_reset import timed_us
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
        raise SystemExit("bench_layer_norm.py needs a GPU (or --vgpr)")
    dev = torch.device("cuda", 0)
    learners = {}
    for dtype in ("fp32", "bf16"):
        for name, flag in (("default_a", False), ("layer_norm", True), ("default_b", False)):
            cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                        "Learner": {"replay_sample_size": args.batch, "q_target_sync_freq": 2500},
                                        "Replay_Memory": {"soft_capacity": args.replay},
                                        "Runtime": {"dtype": dtype, "seed": 1234, "layer_norm": flag}})
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
           "device": torch.cuda.get_device_name(0)}
    for name, r in rates.items():
        out[name] = {"runs": r, "median": float(np.median(r)), "min": min(r), "max": max(r)}
    for dtype in ("fp32", "bf16"):
        a, b, x = (out[f"{dtype}_{k}"]["median"] for k in ("default_a", "default_b", "layer_norm"))
        out[f"{dtype}_aa_spread"] = round(abs(a - b), 1)
        out[f"{dtype}_layer_norm_vs_default_mean"] = round(x - 0.5 * (a + b), 1)
        out[f"{dtype}_layer_norm_us_per_update"] = round(1e6 / x - 1e6 / (0.5 * (a + b)), 2)
    # the isolated launches, last: the backward rewrites dH in place
    for dtype in ("fp32", "bf16"):
        on, off = learners[f"{dtype}_layer_norm"], learners[f"{dtype}_default_a"]
        out[f"{dtype}_fc_fwd_ln_us"] = timed_us(lambda: _fc(on), args.launches)
        out[f"{dtype}_fc_fwd_plain_us"] = timed_us(lambda: _fc(off), args.launches)
        out[f"{dtype}_ln_bwd_reduce_us"] = timed_us(lambda: (on._ln_backward(), on.ops.fc_ln_reduce(on._ln_tok)),
                                                    args.launches)
        out[f"{dtype}_ln_rstd_mean"] = on.last_metrics()["ln_rstd_mean"]
    print(json.dumps(out), flush=True)


def _fc(L) -> None:
    """The fc forward of a learner's 3 B rows alone: GEMM + its (LayerNorm) epilogue, separate launches."""
    sp, n = L.split, 3 * L.B
    wfc, wfc_lo, bfc, wfc_t, wfc_t_lo, bfc_t = L._fc_weights()
    L.ops.fc_fwd(L.y3.reshape(n, 3136), wfc, bfc, L.h, wfc_t, bfc_t, L._rows_first, **L._ln_kw(L.B),
                 **L._lo(x_lo=sp and L.y3_lo.reshape(n, 3136), w_lo=wfc_lo, w2_lo=wfc_t_lo, out_lo=L.h_lo))


if __name__ == "__main__":
    main()
