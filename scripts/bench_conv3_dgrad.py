#!/usr/bin/env python
"""Isolated time of the split-mode conv3 data-gradient launch: the generic implicit GEMM
against the image-resident kernel (csrc/conv3_dgrad_img_split.hip), same session, same buffers.
Each measurement is one HIP-graph replay of --launches back-to-back launches between two
events (no host launch gaps), after a warm-up replay; --reps interleaved repeats.
    python scripts/bench_conv3_dgrad.py [--images 512 256 146 74] [--launches 50] [--reps 7] [--grid 0]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[512, 256, 146, 74])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--grid", type=int, default=0)
    a = ap.parse_args()
    from apex_dqn_amd.ops import _lib as L
    from apex_dqn_amd.ops import conv as C
    from apex_dqn_amd.ops.switches import SW
    lib = L.require_kernels()
    dev = torch.device("cuda", 0)
    have_img = hasattr(lib, "apex_conv3_dgrad_img_split")
    for N in a.images:
        g = torch.Generator(device="cpu").manual_seed(N)

        def planes(x):
            x = x.to(dev)
            hi = x.to(torch.bfloat16)
            return hi, (x - hi.float()).to(torch.bfloat16)

        dyh, dyl = planes(torch.randn(N, 7, 7, 64, generator=g))
        wh, wl = planes(torch.randn(64, 3, 3, 64, generator=g) * 0.04)
        y2 = torch.relu(torch.randn(N, 9, 9, 64, generator=g)).to(dev, torch.bfloat16)
        outs = {k: (torch.empty(N, 9, 9, 64, dtype=torch.bfloat16, device=dev),
                    torch.empty(N, 9, 9, 64, dtype=torch.bfloat16, device=dev)) for k in ("generic", "img")}

        def launch(name):
            hi, lo = outs[name]
            if name == "img":
                C.conv3_dgrad_img_split(lib, dyh, dyl, wh, wl, y2, hi, lo, grid=a.grid)
            else:
                SW.conv3_dgrad_img_split = False
                C.conv3_dgrad(lib, dyh, wh, y2, hi, dy_lo=dyl, w_lo=wl, out_lo=lo)

        names = ("generic", "img") if have_img else ("generic",)
        graphs = {}
        side = torch.cuda.Stream()
        for name in names:
            with torch.cuda.stream(side):
                launch(name)
                side.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=side):
                    for _ in range(a.launches):
                        launch(name)
                graphs[name] = gr
        same = have_img and all(torch.equal(x.view(torch.int16), y.view(torch.int16))
                                for x, y in zip(outs["generic"], outs["img"]))
        res = {k: [] for k in names}
        for name in graphs:
            graphs[name].replay()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, gr in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gr.replay()
                e1.record()
                torch.cuda.synchronize()
                res[name].append(round(1e3 * e0.elapsed_time(e1) / a.launches, 2))
        out = {"images": N, "grid": a.grid, "launches_per_measurement": a.launches, "planes_bit_equal": same,
               "generic_us": res["generic"]}
        if have_img:
            out["img_us"] = res["img"]
            out["median_ratio"] = round(sorted(res["generic"])[a.reps // 2] / sorted(res["img"])[a.reps // 2], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
