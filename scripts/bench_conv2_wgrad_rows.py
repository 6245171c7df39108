#!/usr/bin/env python
"""Isolated time of the split-mode conv2 weight-gradient launch: the generic implicit GEMM
against the row-resident kernel (csrc/conv2_wgrad_rows.hip), same session, same buffers.
Each measurement is one HIP-graph replay of --launches back-to-back launches between two
events (no host launch gaps), after a warm-up replay; --reps interleaved repeats.
    python scripts/bench_conv2_wgrad_rows.py [--images 512] [--launches 50] [--reps 7]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[512])
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

        dyh, dyl = planes(torch.randn(N, 9, 9, 64, generator=g))
        yh, yl = planes(torch.relu(torch.randn(N, 20, 20, 64, generator=g)))
        ws = C.Workspace()
        dw, db = torch.empty(64, 4, 4, 64, device=dev), torch.empty(64, device=dev)
        graphs, slabs = {}, {}
        side = torch.cuda.Stream()
        for name, rows_kernel in (("generic", False), ("rows", True)):
            with torch.cuda.stream(side):
                C.conv_wgrad(lib, ws, dyh, yh, 4, 2, dw, db, jobs=[], dy_lo=dyl, x_lo=yl, rows_kernel=rows_kernel)
                side.synchronize()
                slabs[name] = [t.clone() for k, t in ws.bufs.items() if k[0][0] in ("wg", "wgb")]
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=side):
                    for _ in range(a.launches):
                        C.conv_wgrad(lib, ws, dyh, yh, 4, 2, dw, db, jobs=[], dy_lo=dyl, x_lo=yl,
                                     rows_kernel=rows_kernel)
                graphs[name] = gr
        same = all(torch.equal(x, y) for x, y in zip(slabs["generic"], slabs["rows"]))
        res = {"generic": [], "rows": []}
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
        print(json.dumps({"images": N, "launches_per_measurement": a.launches, "slabs_bit_equal": same,
                          "generic_us": res["generic"], "rows_us": res["rows"],
                          "median_ratio": round(sorted(res["generic"])[a.reps // 2] / sorted(res["rows"])[a.reps // 2], 3)}))


if __name__ == "__main__":
    main()
