#!/usr/bin/env python3
"""Cost of the material-record kernel (RT64_ShadeViewRayHitsDevice, csrc/material.hip) next to the surface-record kernel (RT64_ResolveViewRayHitsDevice) and the
walk that found the hits (RT64_TraceViewRaysDevice, closest hit), timed with HIP events around the calls on a torch stream.

    tools/material_query_rate.py [--iters 10] [--scenes sample,many,stress] [--out file.jsonl]

Scenes: the sample (two ray-traced instances), `many` (the sample + 64 small spheres: 66 instances), `stress` (--subdiv 7 --floor-grid 256 of bench.py); each once
as it is with lods = NULL, and once built with generate_mipmaps = 1 and a per-ray lod drawn from [0, 6).

Rays: the 1080p pixel-centre camera rays in 8 x 8 blocks (a wave = one block: one or two instances per wave), and the same rays shuffled (every wave sees every
instance).  One JSON line per scene x lods x order x kernel.  The material line carries Mrecords/s, its time as a fraction of the trace and of the resolve of the
same batch, and the bytes the algorithm needs per record -- 128 B of records (ray + hit in, record out; + 4 B of lod), and per hit 3 x vertexSize, 12 B of
indices and the texels of H4 / H8 / H9 / H10 (4 B a tap; 4 taps under LINEAR, two levels where a lod blends) -- over the kernel's time against the 8 TB/s HBM
peak: an algorithmic figure (caches serve most of those bytes), named so.  Per-kernel times of one run:  rocprofv3 --kernel-trace --stats -- python3 tools/material_query_rate.py"""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from surface_query_rate import W, H, block_order_pixels, many_instances, timed  # noqa: E402

HBM_PEAK = 8.0e12
VERTEX_SIZE = sample_scene.VERTEX_DTYPE.itemsize


def bytes_per_hit(data, lods):
    """The sample's shader on every instance: diffuse, normal and specular texel at the given lod, the diffuse texel again at level 0 (H10)."""
    taps = 4 if data.shader_filter == rt64.SHADER_FILTER_LINEAR else 1
    levels = 2 if (lods and taps == 4) else 1
    return 3 * VERTEX_SIZE + 12 + 4 * taps * (3 * levels + 1)


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
        for with_lods in (False, True):
            s = sample_scene.Rt64Scene(lib, data, W, H, hip_device=0, options={"generate_mipmaps": 1} if with_lods else None)
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
                    lods = (torch.rand(n, generator=g, device="cuda") * 6.0).contiguous() if with_lods else None
                    lod_ptr = lods.data_ptr() if with_lods else None
                    ms_trace = timed(st, a.iters, a.warmup, lambda: lib.TraceViewRaysDevice(s.view, rays.data_ptr(), hits.data_ptr(), n, 0, st.cuda_stream))
                    ms_resolve = timed(st, a.iters, a.warmup, lambda: lib.ResolveViewRayHitsDevice(s.view, rays.data_ptr(), hits.data_ptr(), rec.data_ptr(), n, st.cuda_stream))
                    ms_shade = timed(st, a.iters, a.warmup, lambda: lib.ShadeViewRayHitsDevice(s.view, rays.data_ptr(), hits.data_ptr(), lod_ptr, rec.data_ptr(), n, st.cuda_stream))
                    hit_frac = float((hits[:, 3].view(torch.int32) >= 0).float().mean().item())
                    valid = float((rec[:, 7].view(torch.int32) & rt64.MATERIAL_VALID).ne(0).float().mean().item())
                    for kernel, ms in (("trace_closest", ms_trace), ("resolve", ms_resolve), ("material", ms_shade)):
                        line = {"scene": name, "lods": "per_ray_0_6_mipmaps" if with_lods else "null", "rays": "camera_1080p", "order": order, "count": n, "kernel": kernel,
                                "ms": round(ms, 4), "ns_per_ray": round(ms * 1e6 / n, 4), "hit_fraction": round(hit_frac, 4)}
                        if kernel == "material":
                            per_record = 128 + (4 if with_lods else 0) + hit_frac * bytes_per_hit(data, with_lods)
                            line.update({"valid_fraction": round(valid, 4), "mrecords_per_s": round(n / (ms * 1e-3) / 1e6, 1), "fraction_of_trace": round(ms_shade / ms_trace, 4),
                                         "fraction_of_resolve": round(ms_shade / ms_resolve, 4), "algorithmic_bytes_per_record": round(per_record, 1),
                                         "algorithmic_gb_per_s": round(n * per_record / (ms * 1e-3) / 1e9, 1),
                                         "algorithmic_fraction_of_8TBps_hbm_peak": round(n * per_record / (ms * 1e-3) / HBM_PEAK, 4)})
                        print(json.dumps(line), flush=True)
                        if out:
                            out.write(json.dumps(line) + "\n"); out.flush()
                    del hits, rec
            finally:
                s.close()
                torch.cuda.synchronize()


if __name__ == "__main__":
    main()
