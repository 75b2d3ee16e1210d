#!/usr/bin/env python3
"""Records per second of RT64_TraceViewPointsIndirectDevice (the chain of csrc/indirect.hip around layer_walk_kernel) at 1 and 4 samples, on as many points as a
1080p frame has pixels, timed with HIP events around the calls on a torch stream; beside each, the time the frame's own GI pass took for the same pixels with the
same sample count (RT64_FRAME_STATS.msIndirect of the frame the points were read from).

    tools/indirect_query_rate.py [--iters 10] [--out file.jsonl]

Scene: the sample scene at 1920 x 1080, denoiser off.  Points: the frame's stored SHADING_POSITION / SHADING_NORMAL / INSTANCE_ID of every pixel, row by row, keys =
NULL; a pixel that shows no surface is RT64_GI_POINT_NONE: it keeps its slots in the chain's arrays and is answered without a walk.  One JSON line per measurement.
There is no gate: nothing preceded these kernels.  The call's time holds its host side (one event wait, and per chunk of 2^20 / (16 giSamples) points four launches,
eight with a second bounce); the frame's pass is one to four launches over the whole picture, and its walk keeps only the closest hit where every instance is
opaque.  profiles/indirect_query_rate.txt is the output of one run
with --out, as written."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as graft

graft.load_package()
from sm64rt_legacy_renderer_amd import rt64, sample_scene  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from surface_query_rate import W, H, timed  # noqa: E402

SAMPLES = (1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    lib = rt64.Library()
    out = open(a.out, "a") if a.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n"); out.flush()
    emit({"note": "ms: median over %d calls, each between two HIP events on a caller stream after %d warm-up calls; a call carries its host side inside that window.  "
                  "frame_ms_indirect: RT64_FRAME_STATS.msIndirect of the frame the points were stored by, median over %d frames." % (a.iters, a.warmup, a.iters),
          "source_hash": __import__("bench").source_hash()})
    data = sample_scene.make_sample_scene()
    for samples in SAMPLES:
        s = sample_scene.Rt64Scene(lib, data, W, H, hip_device=0)
        try:
            s.set_view_description(denoiser=False, gi_samples=samples)
            frame_ms = []
            for _ in range(a.iters + 1):
                s.draw()
                frame_ms.append(float(s.stats().msIndirect))
            position, normal, ident = (s.readback(getattr(rt64, "IMAGE_" + k)) for k in ("SHADING_POSITION", "SHADING_NORMAL", "INSTANCE_ID"))
            n = W * H
            pts = np.zeros((n, 8), dtype=np.float32)
            pts[:, 0:3] = np.asarray(position).reshape(n, -1)[:, :3]; pts[:, 4:7] = np.asarray(normal).reshape(n, -1)[:, :3].astype(np.float32)
            pts.view(np.int32)[:, 7] = np.asarray(ident).reshape(n)
            surface = np.asarray(ident).reshape(n) >= 0
            pts.view(np.uint32)[~surface, 3] = rt64.GI_POINT_NONE
            d_pts = torch.from_numpy(pts).cuda()
            records = torch.empty((n, 12), dtype=torch.float32, device="cuda")
            st = torch.cuda.Stream()
            sampling = rt64.GI_SAMPLING(samples, -1, -1, 0)
            ms = timed(st, a.iters, a.warmup, lambda: lib.TraceViewPointsIndirectDevice(s.view, d_pts.data_ptr(), None, C.addressof(sampling), None, records.data_ptr(), n, st.cuda_stream))
            torch.cuda.synchronize()
            rays = int(records.view(torch.int32)[:, 8].sum().item())
            emit({"scene": "sample", "points": "stored by a 1080p frame, row by row", "count": n, "surface_points": int(surface.sum()), "gi_samples": samples, "rays_walked": rays,
                  "ms": round(ms, 4), "records_per_s": round(n / (ms * 1e-3), 0), "ns_per_ray": round(ms * 1e6 / max(rays, 1), 4),
                  "frame_ms_indirect": round(float(np.median(frame_ms[1:])), 4), "over_frame_pass": round(ms / max(float(np.median(frame_ms[1:])), 1e-9), 3)})
        finally:
            s.close()
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
