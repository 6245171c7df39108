#!/usr/bin/env python
"""Isolated time of the split-mode conv3 weight-gradient launch: the generic implicit GEMM
against the image-resident kernel (csrc/conv3_wgrad_img.hip) at several grids, and of the
grad_finalize launch that reduces each one's partial slabs; same session, same buffers.
Each measurement is one HIP-graph replay of --launches back-to-back launches between two
events (no host launch gaps), after a warm-up replay; --reps interleaved repeats.
    python scripts/bench_conv3_wgrad.py [--images 512 256 146 74] [--grids 64 128 256] [--launches 50] [--reps 7]
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
    ap.add_argument("--grids", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from apex_dqn_amd.ops import _lib as L
    from apex_dqn_amd.ops import conv as C
    lib = L.require_kernels()
    dev = torch.device("cuda", 0)
    for N in a.images:
        g = torch.Generator(device="cpu").manual_seed(N)

        def planes(x):
            x = x.to(dev)
            hi = x.to(torch.bfloat16)
            return hi, (x - hi.float()).to(torch.bfloat16)

        dyh, dyl = planes(torch.randn(N, 7, 7, 64, generator=g))
        yh, yl = planes(torch.relu(torch.randn(N, 9, 9, 64, generator=g)))
        ws = C.Workspace()
        names = ["generic"] + [f"img{G}" for G in a.grids if G <= N or G == a.grids[0]]
        outs = {k: (torch.empty(64, 3, 3, 64, device=dev), torch.empty(64, device=dev)) for k in names}
        jobs = {}

        def launch(name, record=False):
            dw, db = outs[name]
            j = []
            if name == "generic":
                C.conv_wgrad(lib, ws, dyh, yh, 3, 1, dw, db, jobs=j, dy_lo=dyl, x_lo=yl, img_kernel=False)
            else:
                C.conv_wgrad(lib, ws, dyh, yh, 3, 1, dw, db, jobs=j, dy_lo=dyl, x_lo=yl, img_kernel=True,
                             img_grid=int(name[3:]))
            if record:
                jobs[name] = j

        graphs = {}
        side = torch.cuda.Stream()
        for name in names:
            with torch.cuda.stream(side):
                launch(name, record=True)
                C.finalize_grads(lib, jobs[name])
                side.synchronize()
                for kind in ("wgrad", "finalize"):
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=side):
                        for _ in range(a.launches):
                            if kind == "wgrad":
                                launch(name)
                            else:
                                C.finalize_grads(lib, jobs[name])
                    graphs[(name, kind)] = gr
        ref = outs["generic"][0].double()
        res = {k: [] for k in graphs}
        for gr in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for key, gr in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gr.replay()
                e1.record()
                torch.cuda.synchronize()
                res[key].append(round(1e3 * e0.elapsed_time(e1) / a.launches, 2))
        for name in names:
            out = {"images": N, "kernel": name, "nsplit": jobs[name][0]["nsplit"],
                   "launches_per_measurement": a.launches, "wgrad_us": res[(name, "wgrad")],
                   "finalize_us": res[(name, "finalize")],
                   "max_diff_vs_generic": float((outs[name][0].double() - ref).abs().max() / ref.abs().max())}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
