#!/usr/bin/env python3
"""Throughput of the ray-query kernel (RT64_TraceViewRaysDevice, csrc/query.hip), timed with HIP events around the call on a torch stream.

    tools/ray_query_rate.py [--iters 10] [--scenes sample,stress] [--out file.jsonl]

One JSON line per case: scene (the sample; the stress scene = --subdiv 7 --floor-grid 256 of bench.py) x rays (1080p pixel-centre camera rays
built on the host from the view's matrices, in row order; 2 M and 16 M rays with uniformly random origins in the scene box and uniformly random
directions) x mode (closest hit, accept-first).  Next to each case: the frame's own primary-visibility kernel at 1080p (device option
fused_lean = 0, so that primary_trace is its own kernel and RT64_FRAME_STATS.msPrimaryTrace is its time alone), per ray."""
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


def scene_box(data):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in data.instances:
        if not (data.meshes[inst.mesh].flags & rt64.MESH_RAYTRACE_ENABLED):
            continue
        p = data.meshes[inst.mesh].vertices["position"][:, :3].astype(np.float64)
        t = np.asarray(inst.transform, dtype=np.float64)
        w = p @ t[:3, :3] + t[3, :3]
        lo, hi = np.minimum(lo, w.min(axis=0)), np.maximum(hi, w.max(axis=0))
    return lo, hi


def random_rays(data, n, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    lo, hi = scene_box(data)
    r = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    lo_t, ext_t = torch.tensor(lo, dtype=torch.float32, device="cuda"), torch.tensor(hi - lo, dtype=torch.float32, device="cuda")
    r[:, 0:3] = lo_t + torch.rand((n, 3), generator=g, device="cuda") * ext_t
    d = torch.randn((n, 3), generator=g, device="cuda")
    r[:, 4:7] = d / d.norm(dim=1, keepdim=True)
    r[:, 3] = 0.0; r[:, 7] = float("inf")
    return r


def frame_primary_trace_ms(lib, data, frames):
    s = sample_scene.Rt64Scene(lib, data, W, H, hip_device=0)
    try:
        s.option("fused_lean", 0)
        for _ in range(5):
            s.draw()
        ms = []
        for _ in range(frames):
            s.draw()
            ms.append(s.stats().msPrimaryTrace)
        return float(np.median(ms))
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="sample,stress")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    lib = rt64.Library()
    out = open(a.out, "a") if a.out else None
    for name in a.scenes.split(","):
        data = sample_scene.make_sample_scene() if name == "sample" else sample_scene.make_sample_scene(subdiv=7, floor_grid=256)
        frame_ms = frame_primary_trace_ms(lib, data, a.iters)
        s = sample_scene.Rt64Scene(lib, data, W, H, hip_device=0)
        try:
            s.draw()
            ys, xs = np.mgrid[0:H, 0:W]
            cases = [("camera_1080p", torch.from_numpy(sample_scene.camera_rays(data, W, H, np.stack([xs.ravel(), ys.ravel()], axis=1))).cuda()),
                     ("random_2M", random_rays(data, 2 << 20, 1)), ("random_16M", random_rays(data, 16 << 20, 2))]
            st = torch.cuda.Stream()
            for rays_name, rays in cases:
                hits = torch.empty_like(rays)
                n = rays.shape[0]
                for mode, flags in (("closest", 0), ("accept_first", rt64.RAY_FLAG_ACCEPT_FIRST_HIT)):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(st):
                        for _ in range(a.warmup):
                            assert lib.TraceViewRaysDevice(s.view, rays.data_ptr(), hits.data_ptr(), n, flags, st.cuda_stream), lib.last_error()
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
                        for e0, e1 in ev:
                            e0.record(st)
                            lib.TraceViewRaysDevice(s.view, rays.data_ptr(), hits.data_ptr(), n, flags, st.cuda_stream)
                            e1.record(st)
                    torch.cuda.synchronize()
                    ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
                    hit_frac = float((hits[:, 3].view(torch.int32) >= 0).float().mean().item())
                    line = {"scene": name, "rays": rays_name, "count": n, "mode": mode, "ms": round(ms, 4), "ns_per_ray": round(ms * 1e6 / n, 4),
                            "grays_per_s": round(n / (ms * 1e-3) / 1e9, 3), "hit_fraction": round(hit_frac, 4),
                            "frame_ms_primary_trace_1080p": round(frame_ms, 4), "frame_ns_per_primary_ray": round(frame_ms * 1e6 / (W * H), 4)}
                    print(json.dumps(line), flush=True)
                    if out:
                        out.write(json.dumps(line) + "\n"); out.flush()
                del hits
        finally:
            s.close()
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
