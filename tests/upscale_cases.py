"""Cases of the temporal upscaler's rule tests (tests/test_upscale_rule.py on the CPU oracle, tests/test_gpu_upscale_rule.py on the GPU), the sessions both sides draw,
and `hold`, which compares UPSCALED of every compared frame with tests/upscale_rule.py.

Every case draws the sample scene's sphere and floor under the sky plane (post_cases._base, no raster instance) with the built-in upscaler at a screen of at most
81 x 47 for at most 34 frames.  Only `aligned` (64 x 40) is a multiple of the kernel's 32 x 8 workgroup; `edge-plus-one` (65 x 41) is one column and one row past it.
A case is a list of frames and the subset that is compared; the others only build history.  The rule predicts frame N from the side's own readbacks of frame N
(OUTPUT_RGBA32F, FLOW, REACTIVE_MASK, LOCK_MASK, DEPTH) and of frame N - 1 (UPSCALED), the display size and the frame's index.  A case asserts from the rule's own
counts that it reaches what it was built for (REACH, over its compared frames; REACH_AT for a count one named frame must show).

`conf_wins` needs 0.1 conf > 1 / (N + 1), that is N >= 10 at any ratio -- a mode case of two or three frames cannot show it -- so `ultra-performance` draws 13 frames (11
of them only build history) and `cap` is required to show it too; the other mode cases draw three.  `restart` changes the mode at frame 2 and the display size at frame 4.
`sharpened` runs on the GPU alone (the oracle has no sharpening pass); on the CPU `history_is_sharpened` is shown on `strafe`."""
import copy

import numpy as np

import mirror_cases as MC
import post_cases as PCS
import primary_cases as PC
import upscale_rule as UR

CASES = ("first", "still", "strafe", "locked", "reactive", "cap", "performance", "ultra-performance", "ultra-quality", "native", "balanced", "aligned", "edge-plus-one",
         "restart", "gi")
GPU_ONLY_CASES = ("sharpened",)

REACH = {
    "first": ("fresh", "taps_clamped_left", "taps_clamped_right", "taps_clamped_top", "taps_clamped_bottom"),
    "still": ("count_wins", "taps_clamped_left", "taps_clamped_right", "taps_clamped_top", "taps_clamped_bottom", "i0_clamped", "k0_clamped"),
    "strafe": ("flow_not_centre", "history_off_screen", "history_clamped_edge", "outside_box", "count_wins"),
    "locked": ("locked_outside_box", "outside_box"), "reactive": ("reactive_wins",), "cap": ("capped", "conf_wins"),
    "performance": ("count_wins",), "ultra-performance": ("conf_wins",), "ultra-quality": ("count_wins",), "native": ("count_wins",), "balanced": ("count_wins",),
    "aligned": ("count_wins",), "edge-plus-one": ("count_wins",), "restart": ("fresh", "count_wins"), "gi": ("count_wins", "flow_not_centre"), "sharpened": ("count_wins", "outside_box"),
}
# frame 0 is jitter phase 0: j.x = 0 and at 1.5 x a third of the columns have r.x on an integer; on one of them float32 and float64 take the floor differently
REACH_AT = {"still": {0: ("on_grid_x", "near_grid_x")}}
MODE_NAMES = {"performance": UR.MODE_PERFORMANCE, "ultra-performance": UR.MODE_ULTRA_PERFORMANCE, "ultra-quality": UR.MODE_ULTRA_QUALITY, "native": UR.MODE_NATIVE,
              "balanced": UR.MODE_BALANCED}
RENDER = {"performance": (40, 23), "ultra-performance": (27, 15), "ultra-quality": (62, 36), "native": (81, 47), "balanced": (47, 27)}          # the table at 81 x 47

# the case built to catch each wrong variant of the rule (tie_takes_last: see tests/test_upscale_rule.py and DESIGN.md)
MUTATION_CASE = {
    "jitter_subtracted": "still", "floor_without_jitter": "still", "distance_from_clamped_index": "still", "sigma_two": "still", "flow_of_centre": "strafe",
    "flow_of_farthest": "strafe", "flow_in_display_pixels": "strafe", "flow_subtracted": "strafe", "masks_of_nearest_depth": "reactive", "history_nearest": "strafe",
    "history_no_half_texel": "strafe", "off_screen_clamped_not_dropped": "strafe", "no_colour_clamp": "strafe", "lock_ignored": "locked", "lock_inverted": "locked",
    "reactive_ignored": "reactive", "conf_dropped": "cap", "one_over_n": "still", "cap_64": "cap", "history_is_sharpened": "strafe",
}
HAND_MADE = ("tie_takes_last",)

ORACLE_IMAGES = {"output": "output", "flow": "flow", "reactive": "reactiveMask", "lock": "lockMask", "depth": "depth", "upscaled": "upscaled", "final": "final"}
GPU_IMAGES = {"output": "OUTPUT_RGBA32F", "flow": "FLOW", "reactive": "REACTIVE_MASK", "lock": "LOCK_MASK", "depth": "DEPTH", "upscaled": "UPSCALED", "final": "FINAL_RGBA8"}
RULE_INPUTS = ("output", "flow", "reactive", "lock", "depth")


def make_case(sample_data, name):
    """dict(name, frames, compared, view: the view description, options: device options the oracle has too, data_at: frame -> SceneData, mode_at: frame -> quality mode,
    size_at: frame -> the screen)."""
    d, sphere, floor = PCS._base(sample_data)
    case = dict(name=name, frames=4, compared=(0, 1, 2, 3), view=dict(di_samples=0, gi_samples=0, max_lights=12), options=dict(max_reflections=2))
    mode, size = (lambda f: UR.MODE_QUALITY), (lambda f: (81, 47))
    still = lambda f: (0.0, 2.0, 10.0)
    eye = still
    strafe = lambda f: (0.25 * max(0, f - 1), 2.0, 10.0)                   # from frame 2
    if name == "first":
        case.update(frames=1, compared=(0,))
    elif name == "still":
        pass
    elif name in ("strafe", "locked", "reactive", "sharpened"):
        MC._add_quad(d, "backdrop", (0.0, 4.0, -4.5), 14.0, 8.0, "camera")
        eye = strafe; case.update(frames=5, compared=(1, 2, 3, 4))
        if name == "locked":
            sphere.material.lockMask = 0.75; floor.material.lockMask = 0.25
        if name == "reactive":
            V3 = type(sphere.material.selfLight)
            floor.material.fogEnabled = 1; floor.material.fogMul = 4000.0; floor.material.fogOffset = -3720.0; floor.material.fogColor = V3(0.5, 0.75, 1.0)
            p = MC._add_quad(d, "pane", (3.5, 1.5, 2.0), 1.5, 1.0, "camera"); p.material.solidAlphaMultiplier = 0.6
            p.material.fogEnabled = 1; p.material.fogMul = 4000.0; p.material.fogOffset = -3720.0; p.material.fogColor = V3(1.0, 0.75, 0.5)
        if name == "sharpened":
            case["view"].update(upscaler_sharpness=1.0)
    elif name == "cap":
        size = lambda f: (33, 19)
        case.update(frames=34, compared=(31, 32, 33))
    elif name in MODE_NAMES:
        mode = lambda f: MODE_NAMES[name]
        if name == "ultra-performance":
            eye = lambda f: (0.25 * max(0, f - 11), 2.0, 10.0); case.update(frames=13, compared=(11, 12))
        else:
            eye = strafe; case.update(frames=3, compared=(1, 2))
    elif name in ("aligned", "edge-plus-one"):
        size = (lambda f: (64, 40)) if name == "aligned" else (lambda f: (65, 41))
        eye = strafe; case.update(frames=3, compared=(1, 2))
    elif name == "restart":
        mode = lambda f: UR.MODE_QUALITY if f < 2 else UR.MODE_PERFORMANCE
        size = lambda f: (81, 47) if f < 4 else (65, 41)
        case.update(frames=6, compared=(1, 2, 3, 4, 5))
    elif name == "gi":
        MC._add_quad(d, "backdrop", (0.0, 4.0, -4.5), 14.0, 8.0, "camera")
        mode = lambda f: UR.MODE_PERFORMANCE
        eye = strafe; case.update(frames=4, compared=(2, 3))
        case["view"].update(gi_samples=1, denoiser=True); case["options"].update(denoiser_mode=1)
    else:
        raise KeyError(name)
    views = [PC._view(eye(f), 0.0) for f in range(case["frames"])]

    def data_at(frame):
        c = copy.copy(d); c.view = views[frame]
        return c
    case.update(data_at=data_at, mode_at=mode, size_at=size)
    return case


def restarts(case, f):
    """The accumulation starts over at frame f: the first frame, or one whose buffers were created again (another render size or display size)."""
    if f == 0:
        return True
    now, before = case["size_at"](f), case["size_at"](f - 1)
    return now != before or UR.quality(case["mode_at"](f), *now)[:2] != UR.quality(case["mode_at"](f - 1), *before)[:2]


def wanted(case):
    """{frame: the images read after it}: UPSCALED behind every frame that is compared or precedes a compared one, the rule's inputs and the back buffer behind a compared one."""
    out = {}
    for n in case["compared"]:
        out[n] = tuple(ORACLE_IMAGES)
        if n > 0 and n - 1 not in case["compared"]:
            out.setdefault(n - 1, ("upscaled",))
    return out


# ---- sessions ---------------------------------------------------------------------------------------------------------------------------------------

def oracle_session(case):
    """{frame: images} as the CPU oracle draws them, with the oracle's own `jitter` of the frame."""
    from oracle import oracle_py
    kw = {PCS.ORACLE_VIEW[k]: (int(v) if isinstance(v, bool) else v) for k, v in case["view"].items() if k in PCS.ORACLE_VIEW}
    kw.update({PCS.ORACLE_OPTIONS[k]: v for k, v in case["options"].items()})
    want, out = wanted(case), {}
    o = oracle_py.OracleScene(case["data_at"](0))
    try:
        for f in range(case["frames"]):
            o.data = case["data_at"](f)
            ref = o.render(*case["size_at"](f), images=f in want, upscaler=UR.UPSCALER_FSR, upscalerMode=case["mode_at"](f), **kw)
            if f in want:
                out[f] = {key: ref[ORACLE_IMAGES[key]] for key in want[f]}
                out[f]["jitter"] = ref["pixelJitter"]
    finally:
        o.close()
    return out


def gpu_session(rt64_lib, case, options=None, band=None):
    """The same frames on the device, with further device options (a launch form).  Returns ({frame: images}, {frame: FRAME_STATS of the compared frames})."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    want, out, stats = wanted(case), {}, {}
    s = sample_scene.Rt64Scene(rt64_lib, case["data_at"](0), *case["size_at"](0), hip_device=0)
    try:
        for key, v in dict(case["options"], **(options or {})).items():
            assert s.option(key, v), key
        if band:
            s.set_tile(*band)
        for f in range(case["frames"]):
            if f == 0 or case["mode_at"](f) != case["mode_at"](f - 1):
                s.set_view_description(upscaler=rt64.UPSCALER_FSR, upscaler_mode=case["mode_at"](f), **case["view"])
            if f > 0 and case["size_at"](f) != case["size_at"](f - 1):
                rt64_lib.SetDeviceSize(s.device, *case["size_at"](f))
            s.data = case["data_at"](f)
            s.draw()
            if f in want:
                out[f] = {key: s.readback(getattr(rt64, "IMAGE_" + GPU_IMAGES[key])) for key in want[f]}
                if f in case["compared"]:
                    stats[f] = s.stats()
        return out, stats
    finally:
        s.close()


# ---- holding a side to the rule ---------------------------------------------------------------------------------------------------------------------

def rule_inputs(case, frames, n):
    img = frames[n]
    w, h = case["size_at"](n)
    rw, rh, phases = UR.quality(case["mode_at"](n), w, h)
    prev = None if restarts(case, n) else frames[n - 1]["upscaled"]
    return dict(images=[img[k] for k in RULE_INPUTS], jitter=UR.jitter(n, phases), prev=prev, display=(w, h), render=(rw, rh))


def run_rule(case, frames, n, mutate=None):
    i = rule_inputs(case, frames, n)
    return UR.upsample(*i["images"], i["jitter"], i["prev"], i["display"], mutate=mutate)


def hold(case, frames, side, rules=None, log=print):
    """Every compared frame against the rule; asserts the conditions of the tests and returns the report rows.  rules: a cache {input bytes: rule result}."""
    rules = {} if rules is None else rules
    name = case["name"]
    rows, total = [], {}
    for n in case["compared"]:
        i = rule_inputs(case, frames, n)
        img = frames[n]
        w, h = i["display"]
        out = np.asarray(img["output"])
        assert (out.shape[1], out.shape[0]) == i["render"], (name, n, out.shape, i["render"])               # the render size is the table's
        assert name not in RENDER or i["render"] == RENDER[name], (name, i["render"])
        assert np.asarray(img["upscaled"]).shape == (h, w, 4) and np.asarray(img["final"]).shape == (h, w, 4), (name, n)
        if "jitter" in img:                                                                                     # the oracle says which jitter it drew with
            assert tuple(np.float32(img["jitter"])) == tuple(np.float32(i["jitter"])), (name, n, img["jitter"], i["jitter"])
        fl = np.asarray(img["flow"], dtype=np.float32)
        assert np.array_equal(fl.astype(np.float16).astype(np.float32), fl), (name, n, "FLOW is not float16")
        for k in ("reactive", "lock"):
            m = np.asarray(img[k], dtype=np.float32)
            assert np.array_equal(np.round(m.astype(np.float64) * 255.0).astype(np.float32) / np.float32(255.0), m), (name, n, k, "not the float32 of a UNORM8")
        key = UR.key(*i["images"], i["prev"], np.array(i["jitter"]), np.array(i["display"]))
        if key not in rules:
            rules[key] = UR.upsample(*i["images"], i["jitter"], i["prev"], i["display"])
        rule = rules[key]
        counts = rule["info"]["counts"]
        c = UR.compare(img["upscaled"], rule)
        bad, count_bad = int(c["bad"].sum()), int(c["count_bad"].sum())
        rows.append("upscale_rule %-24s %-17s frame %2d render %dx%d ratio=%.6f/%.6f widest_bound=%.2e count_dev=%.2e bad=%d count_bad=%d not_decided=%d not_covered=%d counts %s"
                    % (side, name, n, i["render"][0], i["render"][1], c["largest"], c["mean"], float(rule["bound"].max()), float(c["count_dev"].max()), bad, count_bad,
                       counts["not_decided"], counts["not_covered"], {k: v for k, v in counts.items() if v and k not in ("not_decided", "not_covered", "pixels")}))
        log(rows[-1])
        assert counts["not_covered"] == 0 and counts["not_decided"] == 0, (name, n, counts)
        assert bad == 0 and c["largest"] < 1.0, (name, n, bad, c["largest"])
        assert count_bad == 0, (name, n, count_bad, float(c["count_dev"].max()))
        up = np.asarray(img["upscaled"])
        assert (up[..., 3][rule["fresh"]] == 1.0).all() and (up[..., 3][rule["masks"]["capped"] & rule["count_exact"]] == 32.0).all(), (name, n)
        if restarts(case, n):
            assert counts["fresh"] == w * h and (up[..., 3] == 1.0).all(), (name, n, counts["fresh"])
        assert rule["covered"][:, -1].all() and rule["covered"][-1].all() and not c["bad"][:, -1].any() and not c["bad"][-1].any()        # the last column and row are held
        for k in REACH_AT.get(name, {}).get(n, ()):
            assert counts[k] > 0, (name, n, k, counts)
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    for k in REACH[name]:
        assert total.get(k, 0) > 0, (name, k, total)
    return rows
