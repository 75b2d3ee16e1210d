#!/usr/bin/env python3
"""Records per second of the two kernels of csrc/footprint.hip on device arrays -- RT64_GenerateViewCameraRaysDevice (camera_ray_kernel) and
RT64_FootprintViewRayHitsDevice (hit_footprint_kernel) -- next to RT64_ResolveViewRayHitsDevice (hit_surface_kernel) on the same batch and the same build,
timed with HIP events around the calls on a torch stream.

    tools/footprint_query_rate.py [--iters 10] [--scenes sample,many] [--out file.jsonl]

Scenes: the sample (two ray-traced instances) and `many` (the sample + 64 small spheres: 66 instances), as tools/surface_query_rate.py has them.

Rays: the library's own camera rays of every 1080p pixel in 8 x 8 blocks (a wave = one block: one or two instances per wave), and the same rays shuffled (every
wave sees every instance and gathers its vertices from all over the meshes).  One JSON line per scene x order x kernel, with the bytes a record moves through the
caller's arrays (camera rays: 8 in, 32 + 64 out; footprints: 32 + 64 + 32 in, 64 out; surface records: 32 + 32 in, 64 out) as GB/s.  There is no gate: nothing
preceded these kernels.  Per-kernel times of one run:  rocprofv3 --kernel-trace --stats -- python3 tools/footprint_query_rate.py"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="sample,many")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    lib = rt64.Library()
    out = open(a.out, "a") if a.out else None
    pixels = torch.from_numpy(block_order_pixels().astype(np.int32)).cuda()
    n = pixels.shape[0]
    for name in a.scenes.split(","):
        data = sample_scene.make_sample_scene()
        if name == "many":
            data = many_instances(data)
        s = sample_scene.Rt64Scene(lib, data, W, H, hip_device=0)
        try:
            s.draw()
            st = torch.cuda.Stream()
            blocks = torch.empty((n, 8), dtype=torch.float32, device="cuda"); bdiffs = torch.empty((n, 16), dtype=torch.float32, device="cuda")
            ms_rays = timed(st, a.iters, a.warmup, lambda: lib.GenerateViewCameraRaysDevice(s.view, pixels.data_ptr(), blocks.data_ptr(), None, n, st.cuda_stream))
            ms_rays_diffs = timed(st, a.iters, a.warmup, lambda: lib.GenerateViewCameraRaysDevice(s.view, pixels.data_ptr(), blocks.data_ptr(), bdiffs.data_ptr(), n, st.cuda_stream))
            ms_rays_index = timed(st, a.iters, a.warmup, lambda: lib.GenerateViewCameraRaysDevice(s.view, None, blocks.data_ptr(), bdiffs.data_ptr(), n, st.cuda_stream))
            assert lib.GenerateViewCameraRaysDevice(s.view, pixels.data_ptr(), blocks.data_ptr(), bdiffs.data_ptr(), n, st.cuda_stream)
            torch.cuda.synchronize()
            lines = [("camera_rays", "blocks_8x8", ms_rays, 8 + 32, {}), ("camera_rays+diffs", "blocks_8x8", ms_rays_diffs, 8 + 96, {}), ("camera_rays+diffs pixels=NULL", "row_major", ms_rays_index, 96, {})]
            g = torch.Generator(device="cuda"); g.manual_seed(1)
            perm = torch.randperm(n, generator=g, device="cuda")
            for order, rays, diffs in (("blocks_8x8", blocks, bdiffs), ("shuffled", blocks[perm].contiguous(), bdiffs[perm].contiguous())):
                hits = torch.empty_like(rays)
                rec = torch.empty((n, 16), dtype=torch.float32, device="cuda")
                assert lib.TraceViewRaysDevice(s.view, rays.data_ptr(), hits.data_ptr(), n, 0, st.cuda_stream)
                ms_resolve = timed(st, a.iters, a.warmup, lambda: lib.ResolveViewRayHitsDevice(s.view, rays.data_ptr(), hits.data_ptr(), rec.data_ptr(), n, st.cuda_stream))
                ms_foot = timed(st, a.iters, a.warmup, lambda: lib.FootprintViewRayHitsDevice(s.view, rays.data_ptr(), diffs.data_ptr(), hits.data_ptr(), rec.data_ptr(), n, st.cuda_stream))
                valid = float((rec[:, 7].view(torch.int32) & rt64.FOOTPRINT_VALID).ne(0).float().mean().item())
                ms_foot_bare = timed(st, a.iters, a.warmup, lambda: lib.FootprintViewRayHitsDevice(s.view, rays.data_ptr(), None, hits.data_ptr(), rec.data_ptr(), n, st.cuda_stream))
                extra = {"valid_fraction": round(valid, 4)}
                lines += [("resolve", order, ms_resolve, 128, extra), ("footprint", order, ms_foot, 192, dict(extra, fraction_of_resolve=round(ms_foot / ms_resolve, 4))),
                          ("footprint diffs=NULL", order, ms_foot_bare, 128, dict(extra, fraction_of_resolve=round(ms_foot_bare / ms_resolve, 4)))]
                del hits, rec
            for kernel, order, ms, nbytes, extra in lines:
                line = {"scene": name, "rays": "camera_1080p", "order": order, "count": n, "kernel": kernel, "ms": round(ms, 4), "ns_per_record": round(ms * 1e6 / n, 4),
                        "records_per_s": round(n / (ms * 1e-3), 0), "bytes_per_record": nbytes, "gb_per_s": round(n * nbytes / (ms * 1e-3) / 1e9, 1)}
                line.update(extra)
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n"); out.flush()
        finally:
            s.close()
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
