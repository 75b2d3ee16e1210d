#!/usr/bin/env python3
"""Rays per second of RT64_TraceViewRayLayersDevice (layer_walk_kernel of csrc/layers.hip) at maxLayers 1, 4 and 16, next to RT64_TraceViewRaysAlphaDevice on the
same rays -- alpha_query_kernel, the yardstick: the closest accepted hit, no list -- and of RT64_WeighViewRayLayersDevice (layer_weight_kernel) on the lists just
built, timed with HIP events around the calls on a torch stream.

    tools/layers_query_rate.py [--iters 30] [--count 1048576] [--out file.jsonl]

Scenes: the sheet stack of tests/layers_cases.py (`instances_20`: twenty translucent sheets over the sample scene's floor, every ray through the stack fills its list)
and the sample scene (every instance opaque: a list is one entry long).  Rays: the library's own camera rays of `count` 1080p pixels in 8 x 8 blocks, the first ones
of the frame on the stack (the upper rows, where the sheets are) and the last ones on the sample scene (the floor and the sphere).  One JSON line per measurement, with
the bytes a ray moves through the caller's arrays (alpha: 32 in, 32 out; walk: 32 in, maxLayers x 32 + 16 out; weigh: 32 + maxLayers x 32 in, maxLayers x 4 + 16 out).
There is no gate: nothing preceded these kernels.  The first line of a run is a note on what the times contain.  profiles/layers_query_rate.txt is the output of one
run with --out, as written."""
import argparse
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
from surface_query_rate import W, H, block_order_pixels, timed  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import layers_cases  # noqa: E402

LAYERS = (1, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    lib = rt64.Library()
    out = open(a.out, "a") if a.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n"); out.flush()
    emit({"note": "ms: median over %d calls, each between two HIP events on a caller stream after %d warm-up calls.  A call carries its host side inside that window: every "
                  "entry point records an event on the device's stream and makes the caller's stream wait for it before it launches, so over_alpha_walk is a ratio of call "
                  "times, not of kernel times." % (a.iters, a.warmup), "source_hash": __import__("bench").source_hash()})
    sample = sample_scene.make_sample_scene()
    order = block_order_pixels()
    scenes = (("sheet stack, 20 sheets", layers_cases.case(sample, "instances_20")[0], order[:a.count]), ("sample", sample, order[-a.count:]))
    for name, data, px in scenes:
        pixels = torch.from_numpy(np.ascontiguousarray(px).astype(np.int32)).cuda()
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
            ms_alpha = timed(st, a.iters, a.warmup, lambda: lib.TraceViewRaysAlphaDevice(s.view, rays.data_ptr(), None, hits.data_ptr(), n, rt64.RAY_FLAG_CULL_BACK_FACING, st.cuda_stream))
            lines = [("alpha_walk", 1, ms_alpha, 64, {})]
            for m in LAYERS:
                lh, ll, lw, lc = new(m, n, 8), new(n, 4), new(m, n), new(n, 4)
                ms_walk = timed(st, a.iters, a.warmup, lambda: lib.TraceViewRayLayersDevice(s.view, rays.data_ptr(), None, m, lh.data_ptr(), ll.data_ptr(), n, rt64.RAY_FLAG_CULL_BACK_FACING, st.cuda_stream))
                ms_weigh = timed(st, a.iters, a.warmup, lambda: lib.WeighViewRayLayersDevice(s.view, rays.data_ptr(), lh.data_ptr(), None, m, lw.data_ptr(), lc.data_ptr(), n, st.cuda_stream))
                torch.cuda.synchronize()
                counts = ll.view(torch.int32)[:, 0].float()
                extra = {"mean_layers_written": round(float(counts.mean().item()), 3), "rays_with_a_list": round(float((counts > 0).float().mean().item()), 4)}
                lines += [("layer_walk", m, ms_walk, 32 + 32 * m + 16, dict(extra, over_alpha_walk=round(ms_walk / ms_alpha, 4))),
                          ("layer_weigh", m, ms_weigh, 32 + 32 * m + 4 * m + 16, dict(extra, mean_shaded=round(float(lc.view(torch.int32)[:, 2].float().mean().item()), 3)))]
                del lh, ll, lw, lc
            for kernel, m, ms, nbytes, extra in lines:
                line = {"scene": name, "rays": "camera_1080p blocks_8x8", "count": n, "what": kernel, "max_layers": m, "ms": round(ms, 4), "ns_per_ray": round(ms * 1e6 / n, 4),
                        "rays_per_s": round(n / (ms * 1e-3), 0), "bytes_per_ray": nbytes, "gb_per_s": round(n * nbytes / (ms * 1e-3) / 1e9, 1)}
                line.update(extra)
                emit(line)
        finally:
            s.close()
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
