"""Host vs device Atari preprocessing for the GPU actors (Runtime.atari_preprocess) on one MI355X.

Two measurements, each a child process of this script under its own ``timeout`` (a part that
fails or runs out of time ends the script; nothing more is started on the GPU after it):

* ``actor``  -- one ``GpuActorGroup`` of E ``fake_ale`` envs, no learner running, stepped for a
  fixed number of steps in host mode (the fp32 numpy preprocessing in the actor's host thread,
  84x84 frames H2D) and in device mode (raw frame pairs H2D, csrc/atari_frames.hip), alternating
  rounds in ONE process.  Reports env steps/s per round and the host time per group step split
  into env (emulators + wrapper), append (staging + H2D enqueue + kernel launch), policy
  (inference launch and the wait for q / actions) and the rest (n-step builder, inserts).
* ``kernel`` -- ``apex_atari_frames`` alone at n = E from HIP events over 50 launches, its
  achieved bytes/s (n x 208 656 bytes moved: two raw frames in, one 84x84 frame out), and the
  H2D copy of the same raw pairs from pinned memory for scale.

    python scripts/bench_actor_preprocess.py --out bench_out/atari_preprocess_device.md
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_PAIR = 2 * 210 * 160 * 3 + 84 * 84       # 208 656


class _Timer:
    """Accumulates the wall time of a wrapped callable."""

    def __init__(self, fn):
        self.fn, self.total = fn, 0.0

    def __call__(self, *a, **kw):
        t0 = time.perf_counter()
        try:
            return self.fn(*a, **kw)
        finally:
            self.total += time.perf_counter() - t0


def _make_group(mode: str, E: int, device):
    import torch
    from apex_dqn_amd.actors.gpu_actor import make_gpu_actor_group
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "PongNoFrameskip-v4"},
                                "Actor": {"num_actors": E},
                                "Runtime": {"use_graphs": False, "env_backend": "fake_ale",
                                            "atari_preprocess": mode}})
    torch.manual_seed(0)
    rp = GpuReplayShard(65536, 65536, 32768, 4, device=device)
    learner = FusedNatureLearner(cfg, device, rp)
    grp = make_gpu_actor_group(cfg, learner, rp, E, pipeline=1)
    timers = {"env": _Timer(grp.env.step), "policy": _Timer(grp.policy),
              "append": _Timer(rp.append_raw_frames if mode == "device" else rp.append_frames)}
    grp.env.step = timers["env"]
    grp.policy = timers["policy"]
    setattr(rp, "append_raw_frames" if mode == "device" else "append_frames", timers["append"])
    return grp, timers


def part_actor(args) -> dict:
    import torch
    device = torch.device("cuda", 0)
    groups = {m: _make_group(m, args.envs, device) for m in ("host", "device")}
    for grp, _ in groups.values():
        for _ in range(args.warmup):
            grp.step()
    torch.cuda.synchronize()
    rounds = {m: [] for m in groups}
    for _ in range(args.rounds):
        for m, (grp, timers) in groups.items():
            for t in timers.values():
                t.total = 0.0
            t0 = time.perf_counter()
            for _ in range(args.steps):
                grp.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ms = {k: 1e3 * t.total / args.steps for k, t in timers.items()}
            ms["step"] = 1e3 * dt / args.steps
            ms["rest"] = ms["step"] - ms["env"] - ms["append"] - ms["policy"]
            rounds[m].append({"env_steps_per_s": args.envs * args.steps / dt, "ms": ms})
    return {"part": "actor", "envs": args.envs, "steps": args.steps, "rounds": rounds,
            "device_name": torch.cuda.get_device_name(0)}


def part_kernel(args) -> dict:
    import torch
    from apex_dqn_amd.ops import _lib
    device = torch.device("cuda", 0)
    lib = _lib.require_kernels()
    n, F, launches = args.envs, 4 * args.envs, 50
    rng = np.random.default_rng(0)
    host = torch.from_numpy(rng.integers(0, 256, (n, 2, 210, 160, 3), dtype=np.uint8)).pin_memory()
    raw = host.to(device)
    ring = torch.zeros(F, 84, 84, dtype=torch.uint8, device=device)
    st = _lib.stream_ptr(device)

    def launch(i):
        _lib.check(lib.apex_atari_frames(raw.data_ptr(), ring.data_ptr(), n, F, (i * n) % F, st), "atari_frames")

    for i in range(5):
        launch(i)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    ev[0].record()
    for i in range(launches):
        launch(i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    us = np.array([1e3 * ev[i].elapsed_time(ev[i + 1]) for i in range(launches)])
    for _ in range(3):
        raw.copy_(host, non_blocking=True)
    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0.record()
    for _ in range(10):
        raw.copy_(host, non_blocking=True)
    c1.record()
    torch.cuda.synchronize()
    h2d_us = 1e3 * c0.elapsed_time(c1) / 10
    return {"part": "kernel", "n": n, "launches": launches, "kernel_us_mean": float(us.mean()),
            "kernel_us_median": float(np.median(us)), "kernel_us_min": float(us.min()),
            "bytes_moved": n * BYTES_PER_PAIR, "kernel_GBps": n * BYTES_PER_PAIR / (np.median(us) * 1e-6) / 1e9,
            "h2d_bytes": int(host.numel()), "h2d_us": h2d_us, "h2d_GBps": host.numel() / (h2d_us * 1e-6) / 1e9}


def _median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def report(actor: dict, kernel: dict) -> str:
    r = actor["rounds"]
    sps = {m: _median([x["env_steps_per_s"] for x in r[m]]) for m in r}
    lines = ["# Atari preprocessing on the host vs on the device (GPU actors)", "",
             f"`scripts/bench_actor_preprocess.py`: one `GpuActorGroup`, E = {actor['envs']} `fake_ale` envs, no "
             f"learner running, {actor['steps']} group steps per round, the two modes alternating in one process "
             f"on one {actor['device_name']}.  `host` is `Runtime.atari_preprocess = \"host\"` (the default), "
             f"`device` moves the max / gray / resize into `csrc/atari_frames.hip`.", "",
             "## env steps/s", "", "| mode | " + " | ".join(f"round {i + 1}" for i in range(len(r["host"]))) +
             " | median |", "|---|" + "---|" * (len(r["host"]) + 1)]
    for m in r:
        lines.append(f"| {m} | " + " | ".join(f"{x['env_steps_per_s']:,.0f}" for x in r[m]) + f" | {sps[m]:,.0f} |")
    lines += ["", f"device / host = {sps['device'] / sps['host']:.2f}x", "",
              "## host time per group step (ms, median over the rounds)", "",
              "| mode | step | env | append | policy | rest |", "|---|---|---|---|---|---|"]
    for m in r:
        med = {k: _median([x["ms"][k] for x in r[m]]) for k in ("step", "env", "append", "policy", "rest")}
        lines.append(f"| {m} | " + " | ".join(f"{med[k]:.3f}" for k in ("step", "env", "append", "policy", "rest")) + " |")
    lines += ["", "env = emulators + wrapper (in host mode the numpy preprocessing is in here); append = pinned "
              "staging, H2D enqueue and the kernel launch; policy = inference launch + the wait for q / actions; "
              "rest = n-step builder and transition inserts.", "",
              f"## `apex_atari_frames` alone (n = {kernel['n']}, HIP events, {kernel['launches']} launches)", "",
              "| | µs | GB/s |", "|---|---|---|",
              f"| kernel, median (mean {kernel['kernel_us_mean']:.1f}, min {kernel['kernel_us_min']:.1f}) | "
              f"{kernel['kernel_us_median']:.1f} | {kernel['kernel_GBps']:.0f} "
              f"({kernel['bytes_moved'] / 1e6:.1f} MB moved) |",
              f"| H2D of the raw pairs from pinned memory | {kernel['h2d_us']:.1f} | {kernel['h2d_GBps']:.1f} "
              f"({kernel['h2d_bytes'] / 1e6:.1f} MB) |", ""]
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("actor", "kernel"), help="run one measurement in this process (child)")
    ap.add_argument("--envs", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default="bench_out/atari_preprocess_device.md")
    args = ap.parse_args()
    if args.part:
        res = part_actor(args) if args.part == "actor" else part_kernel(args)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results = {}
    for part in ("kernel", "actor"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--part", part,
               "--envs", str(args.envs), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--rounds", str(args.rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(f"part {part} failed with exit status {p.returncode}; stopping\n")
            return p.returncode
        results[part] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    text = report(results["actor"], results["kernel"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
        json.dump(results, f, indent=1)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
