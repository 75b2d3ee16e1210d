#!/usr/bin/env python3
"""What the device option generate_mipmaps costs (csrc/mipgen.hip), on one GPU:
  tools/mipgen_cost.py                     RT64_CreateTexture wall time at 32^2 .. 4096^2 with the option off and on, and C2 / C3 frame time of the sample
                                           scene with its RGBA8 textures created with and without chains (the option is set before the textures exist;
                                           bench.py --option sets it after, where it changes nothing)
  tools/mipgen_cost.py --create-once       one mipped texture of every size, nothing else: run under  rocprofv3 --kernel-trace --stats -d DIR -- ...
  tools/mipgen_cost.py --count-launches DIR  launches per texture from that run's kernel trace (a chain ends with its one mipgen_tail_kernel)"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (32, 64, 256, 1024, 4096)


def _lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    graft.load_package()
    from sm64rt_legacy_renderer_amd import rt64
    return rt64, rt64.Library()


def _texture_desc(rt64, img):
    d = rt64.TEXTURE_DESC()
    d.bytes = img.ctypes.data; d.byteCount = img.nbytes; d.format = rt64.TEXTURE_FORMAT_RGBA8
    d.height, d.width = img.shape[:2]; d.rowPitch = img.shape[1] * 4
    return d


def create_times(rt64, lib, reps):
    import numpy as np
    dev = lib.CreateDeviceHeadless(64, 64, 0)
    assert dev, lib.last_error()
    out = {}
    try:
        rng = np.random.default_rng(0)
        for n in SIZES:
            img = rng.integers(0, 256, (n, n, 4), dtype=np.uint8)
            d = _texture_desc(rt64, img)
            row = {}
            for value in (0, 1, 0, 1):             # alternate; the second pass of each is kept (the first warms the staging buffer and the code object)
                assert lib.SetDeviceOption(dev, b"generate_mipmaps", float(value))
                ts = []
                for _ in range(reps if n < 4096 else max(3, reps // 10)):
                    t0 = time.perf_counter()
                    t = lib.CreateTexture(dev, d)
                    ts.append(time.perf_counter() - t0)
                    assert t, lib.last_error()
                    lib.DestroyTexture(t)
                row["on" if value else "off"] = round(sorted(ts)[len(ts) // 2] * 1e6, 1)
            out["%dx%d" % (n, n)] = row
    finally:
        lib.DestroyDevice(dev)
    return out


def frame_times(rt64, lib, steps, rounds):
    from sm64rt_legacy_renderer_amd import sample_scene
    out = {}
    for config in ("C2", "C3"):
        cfg = sample_scene.BENCH_CONFIGS[config]
        ms = {"off": [], "on": []}
        for _ in range(rounds):
            for key, opts in (("off", None), ("on", {"generate_mipmaps": 1})):
                data = sample_scene.make_sample_scene()
                s = sample_scene.Rt64Scene(lib, data, cfg["width"], cfg["height"], hip_device=0, options=opts)
                try:
                    s.set_view_description(gi_samples=cfg["gi_samples"], denoiser=cfg["denoiser"])
                    for _ in range(20):
                        s.draw()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        s.draw()                    # sync_present (default): RT64_DrawDevice returns when the frame is done
                    ms[key].append((time.perf_counter() - t0) * 1e3 / steps)
                finally:
                    s.close()
        out[config] = {k: {"mean_ms": round(sum(v) / len(v), 4), "runs_ms": [round(x, 4) for x in v]} for k, v in ms.items()}
    return out


def create_once(rt64, lib):
    import numpy as np
    dev = lib.CreateDeviceHeadless(64, 64, 0)
    assert dev and lib.SetDeviceOption(dev, b"generate_mipmaps", 1.0)
    rng = np.random.default_rng(0)
    for n in SIZES:
        img = rng.integers(0, 256, (n, n, 4), dtype=np.uint8)
        t = lib.CreateTexture(dev, _texture_desc(rt64, img))
        assert t, lib.last_error()
        lib.DestroyTexture(t)
    lib.DestroyDevice(dev)


def count_launches(trace_dir):
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert path, "no kernel_trace.csv under " + trace_dir
    rows = [r for r in csv.DictReader(open(path[0])) if "mipgen_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per, cur = [], {"grid": 0, "tail": 0, "ns": 0}
    for r in rows:
        cur["grid" if "mipgen_level_kernel" in r["Kernel_Name"] else "tail"] += 1
        cur["ns"] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if "mipgen_tail_kernel" in r["Kernel_Name"]:
            per.append(cur)
            cur = {"grid": 0, "tail": 0, "ns": 0}
    assert len(per) == len(SIZES), per
    return {"%dx%d" % (n, n): {"launches": p["grid"] + p["tail"], "grid": p["grid"], "tail": p["tail"], "kernel_us": round(p["ns"] / 1e3, 1)}
            for n, p in zip(SIZES, per)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--create-once", action="store_true")
    ap.add_argument("--count-launches", metavar="DIR")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.count_launches:
        print(json.dumps({"launches_per_texture": count_launches(args.count_launches)}))
        return
    rt64, lib = _lib()
    if args.create_once:
        create_once(rt64, lib)
        return
    print(json.dumps({"create_texture_us": create_times(rt64, lib, args.reps)}))
    print(json.dumps({"frame_ms": frame_times(rt64, lib, args.steps, args.rounds)}))


if __name__ == "__main__":
    main()
