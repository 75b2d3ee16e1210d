#!/usr/bin/env python3
"""Cost of the walks that honour alpha (RT64_TraceViewRaysAlphaDevice, RT64_TraceViewRayVisibilityDevice, csrc/alpha_query.hip) next to the walk that commits
every intersection (RT64_TraceViewRaysDevice) and to the two-step workaround they replace, timed with HIP events around the calls on a torch stream: the kernel
alone (device arrays), median of --iters calls, every comparison measured twice, alternated (run 0: a b, run 1: a b), so that the spread of a figure stands next to it.

    tools/alpha_query_rate.py [--iters 10] [--scenes sample,fence,many,stress] [--out file.jsonl]

  sample  all instances shadow-opaque, no texture-edge shader: the any-hit never runs.  visibility against accept-first, alpha closest hit against closest hit: the
          price of carrying the any-hit's registers through the same walk.
  fence   tests/alpha_cases.py: three texture-edge layers over the sphere and the floor, seen from above.  alpha closest hit against the workaround: trace, shade,
          re-trace the rays flagged RT64_MATERIAL_CUTOUT from tMin = t, until none is flagged -- on device arrays, every round (and its compaction) counted.
  many    tests/alpha_cases.py: 66 instances, a texture-edge shader on a third of the small spheres; the walk from HBM.  The same comparison.
  stress  --subdiv 7 --floor-grid 256 of bench.py: visibility, one line per ray set.

Rays: the 1080p pixel-centre camera rays in 8 x 8 blocks, the same rays shuffled, and -- for visibility -- rays from the primary hit points to the scene's first
light (tMin = 0.1 + shadowRayBias, tMax = distance - shadowOffset: a frame's shadow rays without the disc sampling).  One JSON line per scene x rays x kernel x run.
Per-kernel times of one run:  rocprofv3 --kernel-trace --stats -- python3 tools/alpha_query_rate.py

The tool sets no time limit of its own.  On a shared GPU run one scene per invocation, each under a limit sized to it, chained so that a failure ends the chain:
    timeout -k 10 240 python3 tools/alpha_query_rate.py --scenes sample --out profiles/alpha_query_rate.jsonl && \
    timeout -k 10 240 python3 tools/alpha_query_rate.py --scenes fence  --out profiles/alpha_query_rate.jsonl && ...   (many, stress)
The fence and the 66-instance scene are the test suite's (tests/alpha_cases.py, tests/material_cases.py): the tool puts tests/ on sys.path to build them, so that
what is timed is what tests/test_gpu_alpha_query.py holds to the rule."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from surface_query_rate import W, H, block_order_pixels, timed  # noqa: E402

FIRST = rt64.RAY_FLAG_ACCEPT_FIRST_HIT


def light_rays(data, rays, hits):
    """From the hit points of `hits` to the first light: a frame's shadow ray for a point light (misses become Q6-invalid rays: tMin > tMax)."""
    L = data.lights[0]
    lp = torch.tensor([L.position.x, L.position.y, L.position.z], device="cuda", dtype=torch.float32)
    p = rays[:, 0:3] + rays[:, 4:7] * hits[:, 0:1]
    to = lp[None, :] - p
    dist = to.norm(dim=1)
    out = torch.zeros_like(rays)
    out[:, 0:3] = p; out[:, 4:7] = to / dist[:, None]
    out[:, 3] = 0.1 + float(data.instances[1].material.shadowRayBias); out[:, 7] = dist - float(L.shadowOffset)
    miss = hits[:, 3].view(torch.int32) < 0
    out[miss] = 0.0; out[miss, 3] = 1.0; out[miss, 6] = 1.0
    return out.contiguous()


def two_step(lib, view, rays, st, work):
    """The workaround on device arrays.  -> (hits, rounds, rays re-traced)"""
    n = rays.shape[0]
    hits, rec = work["hits"], work["rec"]
    assert lib.TraceViewRaysDevice(view, rays.data_ptr(), hits.data_ptr(), n, 0, st.cuda_stream)
    assert lib.ShadeViewRayHitsDevice(view, rays.data_ptr(), hits.data_ptr(), None, rec.data_ptr(), n, st.cuda_stream)
    idx = torch.nonzero(rec[:, 7].view(torch.int32) & rt64.MATERIAL_CUTOUT).squeeze(1)
    rounds = retraced = 0
    cur = None
    while idx.numel():
        rounds += 1; retraced += int(idx.numel())
        sub = (rays[idx] if cur is None else cur).contiguous()
        sub[:, 3] = hits[idx, 0]
        sub_hits, sub_rec = torch.empty_like(sub), torch.empty((sub.shape[0], 16), dtype=torch.float32, device="cuda")
        assert lib.TraceViewRaysDevice(view, sub.data_ptr(), sub_hits.data_ptr(), sub.shape[0], 0, st.cuda_stream)
        assert lib.ShadeViewRayHitsDevice(view, sub.data_ptr(), sub_hits.data_ptr(), None, sub_rec.data_ptr(), sub.shape[0], st.cuda_stream)
        hits[idx] = sub_hits
        again = torch.nonzero(sub_rec[:, 7].view(torch.int32) & rt64.MATERIAL_CUTOUT).squeeze(1)
        idx, cur = idx[again], sub[again]
    return hits, rounds, retraced


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="sample,fence,many,stress")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    lib = rt64.Library()
    out = open(a.out, "a") if a.out else None
    pixels = block_order_pixels()

    def say(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n"); out.flush()

    for name in a.scenes.split(","):
        options = None
        if name == "stress":
            data = sample_scene.make_sample_scene(subdiv=7, floor_grid=256)
        elif name == "sample":
            data = sample_scene.make_sample_scene()
        else:
            import alpha_cases
            data = alpha_cases.fence(sample_scene.make_sample_scene()) if name == "fence" else alpha_cases.many_instances_with_edges(sample_scene.make_sample_scene())
            options = {"lds_cache": 1}
        s = sample_scene.Rt64Scene(lib, data, W, H, hip_device=0, options=options)
        try:
            s.draw()
            blocks = torch.from_numpy(sample_scene.camera_rays(data, W, H, pixels)).cuda()
            g = torch.Generator(device="cuda"); g.manual_seed(1)
            st = torch.cuda.Stream()
            n = blocks.shape[0]
            work = {"hits": torch.empty_like(blocks), "rec": torch.empty((n, 16), dtype=torch.float32, device="cuda")}
            vis = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            hits = work["hits"]
            with torch.cuda.stream(st):
                assert lib.TraceViewRaysDevice(s.view, blocks.data_ptr(), hits.data_ptr(), n, 0, st.cuda_stream)
                st.synchronize()
                to_light = light_rays(data, blocks, hits)
            sets = [("camera_1080p_blocks_8x8", blocks), ("camera_1080p_shuffled", blocks[torch.randperm(n, generator=g, device="cuda")].contiguous())]
            vis_sets = sets + [("to_first_light", to_light)]

            def trace(rays, flags):
                return lambda: lib.TraceViewRaysDevice(s.view, rays.data_ptr(), hits.data_ptr(), n, flags, st.cuda_stream)

            def alpha(rays):
                return lambda: lib.TraceViewRaysAlphaDevice(s.view, rays.data_ptr(), None, hits.data_ptr(), n, 0, st.cuda_stream)

            def visibility(rays):
                return lambda: lib.TraceViewRayVisibilityDevice(s.view, rays.data_ptr(), vis.data_ptr(), n, 0, st.cuda_stream)

            def pair(what, label, rays, kernels, extra=None):
                """kernels: [(name, call)]; alternated twice; one line per kernel and run, the ratio of the first to the second kernel on each."""
                for run in (0, 1):
                    ms = [timed(st, a.iters, a.warmup, call) for _, call in kernels]
                    for (kernel, _), t in zip(kernels, ms):
                        line = {"scene": name, "measure": what, "rays": label, "count": n, "kernel": kernel, "run": run, "ms": round(t, 4), "ns_per_ray": round(t * 1e6 / n, 4)}
                        if len(ms) == 2:
                            line["ratio_%s_over_%s" % (kernels[0][0], kernels[1][0])] = round(ms[0] / ms[1], 4)
                        line.update(extra or {})
                        say(line)

            if name == "stress":
                for label, rays in vis_sets:
                    pair("visibility", label, rays, [("visibility", visibility(rays))])
                continue
            if name == "sample":
                for label, rays in vis_sets:          # 1.
                    pair("visibility_vs_accept_first", label, rays, [("visibility", visibility(rays)), ("trace_accept_first", trace(rays, FIRST))])
                for label, rays in sets:              # 3.
                    pair("alpha_closest_vs_closest", label, rays, [("alpha_closest", alpha(rays)), ("trace_closest", trace(rays, 0))])
                continue
            for label, rays in sets:                  # 2.
                with torch.cuda.stream(st):
                    want, rounds, retraced = two_step(lib, s.view, rays, st, work)
                    want = want.clone()
                    assert alpha(rays)()
                    st.synchronize()
                    same = bool((hits[:, :5].view(torch.int32) == want[:, :5].view(torch.int32)).all().item())
                extra = {"rounds": rounds, "rays_retraced": retraced, "same_hits": same, "hit_fraction": round(float((want[:, 3].view(torch.int32) >= 0).float().mean().item()), 4)}
                pair("alpha_closest_vs_two_step", label, rays, [("alpha_closest", alpha(rays)), ("two_step_workaround", lambda: two_step(lib, s.view, rays, st, work) is not None)], extra)
                pair("alpha_closest_vs_closest", label, rays, [("alpha_closest", alpha(rays)), ("trace_closest", trace(rays, 0))])
            for label, rays in vis_sets[:2]:
                pair("visibility_vs_accept_first", label, rays, [("visibility", visibility(rays)), ("trace_accept_first", trace(rays, FIRST))])
        finally:
            s.close()
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
