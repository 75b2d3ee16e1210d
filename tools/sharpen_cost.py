#!/usr/bin/env python3
"""Frames of the sample scene behind the built-in upscaler with RT64_VIEW_DESC.upscalerSharpness set, for a kernel trace of rcas_sharpen_kernel
(rules S1-S7) beside its sibling taa_upsample_kernel:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/sharpen_cost.py --size 1920x1080 --size 3840x2160
Each size draws --frames frames in a device of its own (upscalerMode AUTO: quality at 1080p, performance at 4K); the kernel's grid tells the sizes
apart in the trace.  Prints one JSON line per size with the host-side frame time, which is NOT the kernel's time."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from sm64rt_legacy_renderer_amd import rt64, sample_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", action="append", default=[])
ap.add_argument("--frames", type=int, default=60)
ap.add_argument("--sharpness", type=float, default=1.0)
a = ap.parse_args()
lib = rt64.Library()
data = sample_scene.make_sample_scene()
for size in a.size or ["1920x1080", "3840x2160"]:
    w, h = (int(v) for v in size.split("x"))
    s = sample_scene.Rt64Scene(lib, data, w, h, hip_device=0)
    try:
        s.set_view_description(upscaler=rt64.UPSCALER_FSR, upscaler_mode=rt64.UPSCALER_MODE_AUTO, upscaler_sharpness=a.sharpness)
        for _ in range(8):
            s.draw()
        s.readback(rt64.IMAGE_FINAL_RGBA8)
        t0 = time.perf_counter()
        for _ in range(a.frames):
            s.draw()
        sharp = s.readback(rt64.IMAGE_SHARPENED) if a.sharpness > 0 else s.readback(rt64.IMAGE_UPSCALED)
        ms = (time.perf_counter() - t0) * 1e3 / a.frames
        print(json.dumps({"display": [w, h], "render": [s.stats().width, s.stats().height], "sharpness": a.sharpness, "frames": a.frames,
                          "host_ms_per_frame_with_one_readback": round(ms, 4), "image_mean": float(sharp[..., :3].mean())}), flush=True)
    finally:
        s.close()
