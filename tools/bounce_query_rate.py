#!/usr/bin/env python3
"""Rays per second of RT64_TraceViewRayMirrorChainsDevice (mirror_chain_kernel of csrc/bounce.hip) at depth 1, 2 and 4, next to (a) RT64_TraceViewRaysAlphaDevice
alone on the same rays -- alpha_query_kernel, the yardstick: a chain of depth 1 is that walk plus one record -- and (c) the same chains as iterated device calls
(RT64_TraceViewRaysAlphaDevice + RT64_BounceViewRayHitsDevice per segment, the next segment on the reflected rays), timed with HIP events around the calls on a
torch stream.

    tools/bounce_query_rate.py [--iters 30] [--count 1048576] [--out file.jsonl]

Scene: the sample scene with the floor mirrored (reflectionFactor 0.3).  Rays: the library's own camera rays of the last `count` 1080p pixels in 8 x 8 blocks (the lower rows of the frame, where the floor and the sphere are).
The iterated form walks every reflected ray, also those of hits that are no mirror (their walk is real; only a miss's all-zero ray costs nothing): a host that
wants less compacts between the calls, which is the round trip the chain call saves.  One JSON line per measurement, with the bytes a ray moves through the
caller's arrays (alpha: 32 in, 32 out; chain: 32 in, depth x 64 out; iterated: per segment 32 + 32 through the walk, 64 in and 64 out through the records).  There
is no gate: nothing preceded these kernels.  The first line of a run is a note on what the times contain.  profiles/bounce_query_rate.txt is the output of two runs
into one --out file, as written."""
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
from surface_query_rate import W, H, block_order_pixels, timed  # noqa: E402

DEPTHS = (1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    lib = rt64.Library()
    out = open(a.out, "a") if a.out else None
    data = sample_scene.make_sample_scene()
    data.instances = list(data.instances)
    floor = next(k for k, i in enumerate(data.instances) if i.name == "floor")
    import copy
    data.instances[floor] = copy.copy(data.instances[floor]); data.instances[floor].material = sample_scene.copy_material(data.instances[floor].material)
    data.instances[floor].material.reflectionFactor = 0.3
    pixels = torch.from_numpy(np.ascontiguousarray(block_order_pixels()[-a.count:]).astype(np.int32)).cuda()          # the lower rows: the floor and the sphere on it
    n = pixels.shape[0]
    s = sample_scene.Rt64Scene(lib, data, W, H, hip_device=0)
    try:
        s.draw()
        st = torch.cuda.Stream()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
        rays = new(n, 8)
        assert lib.GenerateViewCameraRaysDevice(s.view, pixels.data_ptr(), rays.data_ptr(), None, n, st.cuda_stream)
        torch.cuda.synchronize()
        hits = new(n, 8)
        ms_alpha = timed(st, a.iters, a.warmup, lambda: lib.TraceViewRaysAlphaDevice(s.view, rays.data_ptr(), None, hits.data_ptr(), n, 0, st.cuda_stream))
        lines = [("alpha_walk", 1, ms_alpha, 64, {})]
        for depth in DEPTHS:
            ch, cb = new(depth, n, 8), new(depth, n, 8)
            ms_chain = timed(st, a.iters, a.warmup, lambda: lib.TraceViewRayMirrorChainsDevice(s.view, rays.data_ptr(), None, depth, ch.data_ptr(), cb.data_ptr(), n, 0, st.cuda_stream))
            torch.cuda.synchronize()
            flags = cb[:, :, 3].view(torch.int32)
            walked = [float(((flags[k] & rt64.BOUNCE_VALID) != 0).float().mean().item()) for k in range(depth)]
            ih, ib, ir = new(depth, n, 8), new(depth, n, 8), new(depth, n, 8)

            def iterated():
                src = rays
                for k in range(depth):
                    if not lib.TraceViewRaysAlphaDevice(s.view, src.data_ptr(), None, ih[k].data_ptr(), n, 0, st.cuda_stream):
                        return 0
                    if not lib.BounceViewRayHitsDevice(s.view, src.data_ptr(), ih[k].data_ptr(), None, ib[k].data_ptr(), ir[k].data_ptr(), None, n, st.cuda_stream):
                        return 0
                    src = ir[k]
                return 1
            ms_iter = timed(st, a.iters, a.warmup, iterated)
            extra = {"hit_fraction_per_segment": [round(x, 4) for x in walked]}
            lines += [("mirror_chain", depth, ms_chain, 32 + 64 * depth, dict(extra, over_alpha_walk=round(ms_chain / ms_alpha, 4))),
                      ("iterated_calls", depth, ms_iter, (64 + 128) * depth, dict(extra, chain_over_iterated=round(ms_chain / ms_iter, 4)))]
            del ch, cb, ih, ib, ir
        note = {"note": "ms: median over %d calls, each between two HIP events on a caller stream after %d warm-up calls.  A call of 60-450 us carries its host side inside that "
                        "window: every entry point records an event on the device's stream and makes the caller's stream wait for it before it launches (the iterated form "
                        "2 x depth times per call), so over_alpha_walk and chain_over_iterated are ratios of call times, not of kernel times." % (a.iters, a.warmup),
                "source_hash": __import__("bench").source_hash()}
        print(json.dumps(note), flush=True)
        if out:
            out.write(json.dumps(note) + "\n")
        for kernel, depth, ms, nbytes, extra in lines:
            line = {"scene": "sample, floor mirrored", "rays": "camera_1080p blocks_8x8", "count": n, "what": kernel, "depth": depth, "ms": round(ms, 4), "ns_per_ray": round(ms * 1e6 / n, 4),
                    "rays_per_s": round(n / (ms * 1e-3), 0), "bytes_per_ray": nbytes, "gb_per_s": round(n * nbytes / (ms * 1e-3) / 1e9, 1)}
            line.update(extra)
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n"); out.flush()
    finally:
        s.close()
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
