#!/usr/bin/env python3
"""Cost of the surface-record kernel (RT64_ResolveViewRayHitsDevice, csrc/surface.hip) next to the walk that found its hits (RT64_TraceViewRaysDevice,
closest hit), timed with HIP events around the calls on a torch stream.

    tools/surface_query_rate.py [--iters 10] [--scenes sample,many,stress] [--out file.jsonl]

Scenes: the sample (two ray-traced instances), `many` (the sample + 64 small spheres: 66 instances), `stress` (--subdiv 7 --floor-grid 256 of bench.py).

Rays: the 1080p pixel-centre camera rays in 8 x 8 blocks (a wave = one block: one or two instances per wave), and the same rays shuffled (every wave
sees every instance and gathers its vertices from all over the meshes).  One JSON line per scene x order x kernel; the resolve line carries its time as
a fraction of the trace of the same batch on the same build.  Per-kernel times of one run:  rocprofv3 --kernel-trace --stats -- python3 tools/surface_query_rate.py"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import __graft_entry__ as graft

graft.load_package()
from sm64rt_legacy_renderer_amd import rt64, sample_scene  # noqa: E402

W, H = 1920, 1080


def block_order_pixels():
    """(N, 2) x, y of every pixel, 8 x 8 blocks in row order, row-major inside a block."""
    by, bx, iy, ix = np.meshgrid(np.arange(H // 8), np.arange(W // 8), np.arange(8), np.arange(8), indexing="ij")
    return np.stack([(bx * 8 + ix).ravel(), (by * 8 + iy).ravel()], axis=1)


def many_instances(data, side=8):
    """The sample scene with side x side small copies of the sphere over the floor: a shuffled wave meets dozens of instances."""
    import copy
    d = copy.copy(data); d.instances = list(data.instances)
    for k in range(side * side):
        i = copy.copy(data.instances[1])
        t = np.eye(4, dtype=np.float32) * np.float32(0.3); t[3, :] = (-7.0 + 2.0 * (k % side), 0.6, -12.0 + 2.0 * (k // side), 1.0)
        i.transform = t; i.previous_transform = t; i.name = "copy%d" % k
        d.instances.append(i)
    return d


def timed(st, iters, warmup, call):
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for _ in range(warmup):
            assert call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in ev:
            e0.record(st)
            call()
            e1.record(st)
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="sample,many,stress")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    lib = rt64.Library()
    out = open(a.out, "a") if a.out else None
    pixels = block_order_pixels()
    for name in a.scenes.split(","):
        data = sample_scene.make_sample_scene(subdiv=7, floor_grid=256) if name == "stress" else sample_scene.make_sample_scene()
        if name == "many":
            data = many_instances(data)
        s = sample_scene.Rt64Scene(lib, data, W, H, hip_device=0)
        try:
            s.draw()
            blocks = torch.from_numpy(sample_scene.camera_rays(data, W, H, pixels)).cuda()
            g = torch.Generator(device="cuda"); g.manual_seed(1)
            orders = (("blocks_8x8", blocks), ("shuffled", blocks[torch.randperm(blocks.shape[0], generator=g, device="cuda")].contiguous()))
            st = torch.cuda.Stream()
            for order, rays in orders:
                n = rays.shape[0]
                hits = torch.empty_like(rays)
                rec = torch.empty((n, 16), dtype=torch.float32, device="cuda")
                ms_trace = timed(st, a.iters, a.warmup, lambda: lib.TraceViewRaysDevice(s.view, rays.data_ptr(), hits.data_ptr(), n, 0, st.cuda_stream))
                ms_resolve = timed(st, a.iters, a.warmup, lambda: lib.ResolveViewRayHitsDevice(s.view, rays.data_ptr(), hits.data_ptr(), rec.data_ptr(), n, st.cuda_stream))
                hit_frac = float((hits[:, 3].view(torch.int32) >= 0).float().mean().item())
                valid = float((rec[:, 3].view(torch.int32) & rt64.SURFACE_VALID).ne(0).float().mean().item())
                for kernel, ms in (("trace_closest", ms_trace), ("resolve", ms_resolve)):
                    line = {"scene": name, "rays": "camera_1080p", "order": order, "count": n, "kernel": kernel, "ms": round(ms, 4), "ns_per_ray": round(ms * 1e6 / n, 4),
                            "hit_fraction": round(hit_frac, 4), "valid_fraction": round(valid, 4)}
                    if kernel == "resolve":
                        line["fraction_of_trace"] = round(ms_resolve / ms_trace, 4)
                        line["gb_per_s_128B_per_ray"] = round(n * 128 / (ms * 1e-3) / 1e9, 1)
                    print(json.dumps(line), flush=True)
                    if out:
                        out.write(json.dumps(line) + "\n"); out.flush()
                del hits, rec
        finally:
            s.close()
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
