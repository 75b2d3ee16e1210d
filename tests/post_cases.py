"""Cases of the Compose and PostProcess rule tests (tests/test_compose_rule.py and tests/test_post_rule.py on the CPU oracle, tests/test_gpu_compose_rule.py and
tests/test_gpu_post_rule.py on the GPU), the sessions both sides draw, and `hold_compose` / `hold_post`, which compare OUTPUT_RGBA32F and FINAL_RGBA8 of the last frame
with tests/compose_rule.py and tests/post_rule.py.

Every case draws the sample scene's sphere and floor (mirror_cases._base, with the sky plane kept) without any raster instance -- `rect-background` alone adds one
background instance -- at a screen of at most 96 x 64 for at most 4 frames.  Only `plain` has a width and a height that are multiples of the image kernels' 32 x 8
workgroup.  A case asserts from the rule's own counts that it reaches what it was built for (REACH: every named count must be > 0, `blur`'s `blurred` more than half
the frame)."""
import copy
import hashlib

import numpy as np

import compose_rule as CR
import mirror_cases as MC
import post_rule as PR
import primary_cases as PC

UPSCALER_FSR, UPSCALER_MODE_QUALITY = 3, 4                 # rt64.UPSCALER_FSR, rt64.UPSCALER_MODE_QUALITY

COMPOSE_CASES = ("plain", "lean", "gaussian", "cutout")
POST_CASES = ("up", "down", "ragged", "blur", "blur-edge", "blur-still", "blur-3", "blur-1", "blur-scaled", "rect", "rect-scissor", "rect-viewport", "rect-background",
              "rect-scaled", "rect-off-screen", "upscaled", "upscaled-blur")
GPU_ONLY_POST_CASES = ("sharpened",)                      # the oracle has no sharpening pass

# what each case must reach, by the rule's counts
REACH = {
    "plain": ("lit", "unlit", "partial", "reflection", "refraction", "transparent"), "lean": ("lit", "unlit"), "gaussian": ("lit", "unlit"),
    "cutout": ("lit", "unlit", "partial", "transparent"),
    "up": ("wrapped_left", "wrapped_right", "wrapped_top", "wrapped_bottom"), "down": (), "ragged": ("wrapped_left", "wrapped_right", "wrapped_top", "wrapped_bottom"),
    "blur": ("blurred",), "blur-edge": ("blurred", "clamped_left", "clamped_right", "edge_blend"), "blur-still": (), "blur-3": ("blurred",), "blur-1": ("blurred",),
    "blur-scaled": ("blurred", "wrapped_left", "wrapped_right"),
    "rect": ("outside_left", "outside_right", "outside_top", "outside_bottom"), "rect-scissor": ("outside_left", "outside_right", "outside_top", "outside_bottom"),
    "rect-viewport": ("outside_left", "outside_right", "outside_top", "outside_bottom"),
    "rect-background": ("outside_left", "outside_right", "outside_top", "outside_bottom"),
    "rect-scaled": ("outside_left", "outside_right", "outside_top", "outside_bottom"),
    "rect-off-screen": ("outside_left", "outside_right", "outside_top", "outside_bottom"), "upscaled": (), "upscaled-blur": ("blurred", "clamped_left", "clamped_right"), "sharpened": (),
}

# the case built to catch each wrong variant of a rule
# (alpha_test_ge -- the branch taken at a = 0 too -- has no case: a pixel with DIFFUSE.a = 0 had no contributing hit (PrimaryRayGen.hlsl:86-192), so its additive images
# are 0 and lerp(d, x, 0) = d: no frame tells the variant from the rule.  tests/test_compose_rule.py pins the sentence on a hand-made image.)
COMPOSE_MUTATION_CASE = {"no_alpha_lerp": "plain", "reflection_dropped": "plain", "indirect_not_f16_on_lean": "lean", "lean_reads_filtered": "lean"}
POST_MUTATION_CASE = {
    "clamp_not_wrap": "up", "no_half_texel": "up", "taps_not_clamped": "blur-edge", "start_not_halved": "blur", "flow_in_pixels": "blur",
    "step_over_samples_minus_one": "blur-3", "flow_nearest_at_screen_size": "blur-scaled", "rect_not_flipped": "rect", "scissor_inclusive": "rect",
    "uv_over_screen_not_viewport": "rect", "outside_left_black_over_background": "rect-background",
}

ORACLE_IMAGES = {"diffuse": "diffuse", "direct": "filteredDirect", "indirect": "filteredIndirect", "direct_raw": "directLight", "reflection": "reflection",
                 "refraction": "refraction", "transparent": "transparent", "output": "output", "final": "final", "flow": "flow", "background": "background",
                 "upscaled": "upscaled"}
GPU_IMAGES = {"diffuse": "DIFFUSE", "direct": "DIRECT_LIGHT_FILTERED", "indirect": "INDIRECT_LIGHT_FILTERED", "direct_raw": "DIRECT_LIGHT_RAW", "reflection": "REFLECTION",
              "refraction": "REFRACTION", "transparent": "TRANSPARENT", "output": "OUTPUT_RGBA32F", "final": "FINAL_RGBA8", "flow": "FLOW", "background": "BACKGROUND",
              "upscaled": "UPSCALED", "sharpened": "SHARPENED"}
ORACLE_VIEW = {"di_samples": "diSamples", "gi_samples": "giSamples", "max_lights": "maxLights", "denoiser": "denoiserEnabled", "resolution_scale": "resolutionScale",
               "motion_blur": "motionBlurStrength", "upscaler": "upscaler", "upscaler_mode": "upscalerMode"}
ORACLE_OPTIONS = {"denoiser_mode": "denoiserMode", "max_reflections": "maxReflections", "motion_blur_samples": "motionBlurSamples", "primary_spp": "primarySpp"}


def _base(sample_data):
    """Sphere and floor, flat colours, the sky plane kept (its pixels have DIFFUSE.a = 0), no raster instance."""
    from sm64rt_legacy_renderer_amd import rt64
    d, sphere, floor = MC._base(sample_data)
    d.sky = sample_data.sky
    d.instances = [i for i in d.instances if d.meshes[i.mesh].flags & rt64.MESH_RAYTRACE_ENABLED]
    floor.material.reflectionFactor = 0.0
    return d, sphere, floor


def make_case(sample_data, name):
    """dict(name, kind: "compose" | "post" | "spp", size: the screen, frames, view: the view description, options: device options the oracle has too, data_at: frame ->
    SceneData, lean: the last frame is a lean one, source: the image PostProcess samples, background, viewport, scissor, render: the render size, ambient)."""
    d, sphere, floor = _base(sample_data)
    case = dict(name=name, kind="post", size=(80, 48), frames=2, view=dict(di_samples=0, gi_samples=0, max_lights=12), options=dict(max_reflections=2), lean=False,
                source="output", background=False, viewport=None, scissor=None, render=None)
    eye = lambda f: (0.0, 2.0, 10.0)
    strafe = lambda f: (0.5 * f, 2.0, 10.0)
    if name == "plain":
        # GI + SVGF, a mirroring floor, a glass sphere, a pane too thin to be the lit hit (alpha 0.4 <= APPLY_LIGHTS_MINIMUM_ALPHA: it goes to gTransparent)
        case.update(kind="compose", size=(64, 40), frames=3)
        case["view"].update(gi_samples=1, denoiser=True); case["options"].update(denoiser_mode=1)
        floor.material.reflectionFactor = 0.3
        sphere.material.refractionFactor = 0.9; sphere.material.solidAlphaMultiplier = 0.6
        p = MC._add_quad(d, "pane", (-3.0, 1.5, 4.0), 1.0, 1.0, "camera"); p.material.solidAlphaMultiplier = 0.4
    elif name == "lean":
        case.update(kind="compose", size=(61, 37), lean=True)
    elif name == "gaussian":
        case.update(kind="compose", size=(61, 37), frames=3)
        case["view"].update(gi_samples=1, denoiser=True); case["options"].update(denoiser_mode=0)
    elif name == "cutout":
        # against the sky (DIFFUSE.a = 0): a lit pane of alpha 0.6 and an unlit one of alpha 0.4, both with 0 < DIFFUSE.a < 1; the second one's colour is in gTransparent
        case.update(kind="compose", size=(61, 37), frames=1)
        a = MC._add_quad(d, "high", (3.0, 6.5, -4.0), 2.0, 1.0, "camera"); a.material.solidAlphaMultiplier = 0.6
        b = MC._add_quad(d, "thin", (-3.0, 6.5, -4.0), 2.0, 1.0, "camera"); b.material.solidAlphaMultiplier = 0.4; b.material.lightGroupMaskBits = 0; MC._colour(b, (255, 204, 0))
    elif name == "spp":
        case.update(kind="spp", size=(61, 37), frames=1); case["options"].update(primary_spp=2)
    elif name == "up":
        case["view"].update(resolution_scale=0.75); case["render"] = (60, 36)
    elif name == "down":
        case.update(size=(61, 37)); case["view"].update(resolution_scale=1.5); case["render"] = (92, 56)
    elif name == "ragged":
        case.update(size=(81, 47)); case["view"].update(resolution_scale=0.6); case["render"] = (49, 28)
    elif name in ("blur", "blur-edge", "blur-3", "blur-1", "blur-scaled", "blur-still"):
        MC._add_quad(d, "backdrop", (0.0, 4.0, -4.5), 14.0, 8.0, "camera")             # fills the rows the sky would leave without flow
        case.update(size=(75, 43), frames=3)
        case["view"].update(motion_blur=4.0 if name == "blur-edge" else 1.0)
        if name != "blur-still":
            eye = strafe
        if name in ("blur-3", "blur-1"):
            case["options"].update(motion_blur_samples=int(name[-1]))
        if name == "blur-scaled":
            case.update(size=(80, 48)); case["view"].update(resolution_scale=0.75); case["render"] = (60, 36)
    elif name in ("rect", "rect-scissor", "rect-viewport", "rect-background", "rect-scaled", "rect-off-screen"):
        if name != "rect-scissor":
            case["viewport"] = (8, 5, 40, 30)
        if name != "rect-viewport":
            case["scissor"] = (12, 9, 30, 20)
        if name == "rect-off-screen":
            # the viewport starts left of and below the screen, the scissor ends right of and above it: columns 30..49, rows 14..27 are inside both
            case["viewport"], case["scissor"] = (-10, -6, 60, 40), (30, 20, 70, 40)
        sphere.viewport, sphere.scissor = case["viewport"], case["scissor"]
        if name == "rect-background":
            case["background"] = True
            PC._add_background(d, sample_data)
        if name == "rect-scaled":
            case["view"].update(resolution_scale=0.75); case["render"] = (60, 36)
    elif name in ("upscaled", "upscaled-blur", "sharpened"):
        eye = lambda f: (0.125 * f, 2.0, 10.0)
        case.update(size=(81, 47), frames=3, source="sharpened" if name == "sharpened" else "upscaled")
        if name == "upscaled-blur":
            MC._add_quad(d, "backdrop", (0.0, 4.0, -4.5), 14.0, 8.0, "camera")
            eye = strafe; case["view"].update(motion_blur=1.0)
        case["view"].update(upscaler=UPSCALER_FSR, upscaler_mode=UPSCALER_MODE_QUALITY)
        if name == "sharpened":
            case["view"].update(upscaler_sharpness=1.0)
    else:
        raise KeyError(name)
    assert d.instances[0] is sphere                 # the first ray-traced instance carries the rectangles
    views = [PC._view(eye(f), 0.0) for f in range(case["frames"])]

    def data_at(frame):
        c = copy.copy(d); c.view = views[frame]
        return c
    case["data_at"] = data_at
    e = d.desc
    case["ambient"] = ((e.ambientBaseColor.x, e.ambientBaseColor.y, e.ambientBaseColor.z), (e.ambientNoGIColor.x, e.ambientNoGIColor.y, e.ambientNoGIColor.z))
    case["motion_blur_samples"] = case["options"].get("motion_blur_samples", 32)          # the library's and the reference's default (rt64_view.cpp:53)
    return case


# ---- sessions ---------------------------------------------------------------------------------------------------------------------------------------

def oracle_session(case, **over):
    """The images of the last frame as the CPU oracle draws them.  over: oracle parameters that replace the case's."""
    from oracle import oracle_py
    kw = {ORACLE_VIEW[k]: (int(v) if isinstance(v, bool) else v) for k, v in case["view"].items() if k in ORACLE_VIEW}
    kw.update({ORACLE_OPTIONS[k]: v for k, v in case["options"].items()})
    kw.update(over)
    o = oracle_py.OracleScene(case["data_at"](0))
    try:
        for f in range(case["frames"]):
            o.data = case["data_at"](f)
            ref = o.render(*case["size"], images=f == case["frames"] - 1, **kw)
    finally:
        o.close()
    return {key: ref[name] for key, name in ORACLE_IMAGES.items()}


def gpu_images_of(case, lean):
    """The readbacks a GPU session makes, in order (at most nine).  The back buffer comes first: on a lean frame every other readback materialises the frame's images."""
    if case["kind"] == "spp":
        return ("final", "output")
    if case["kind"] == "compose":
        return ("final", "diffuse", "direct_raw", "output") if lean else ("final", "diffuse", "direct", "indirect", "reflection", "refraction", "transparent", "output")
    return ("final", "output", "flow") + (("background",) if case["background"] else ()) + ((case["source"],) if case["source"] != "output" else ())


def gpu_session(rt64_lib, case, options=None):
    """The same frames on the device, with further device options (a launch form).  Returns (images, FRAME_STATS of the last frame)."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, case["data_at"](0), *case["size"], hip_device=0)
    try:
        s.set_view_description(**case["view"])
        for key, v in dict(case["options"], **(options or {})).items():
            assert s.option(key, v), key
        for f in range(case["frames"]):
            s.data = case["data_at"](f)
            s.draw()
        st = s.stats()
        return {key: s.readback(getattr(rt64, "IMAGE_" + GPU_IMAGES[key])) for key in gpu_images_of(case, bool(st.leanFrame))}, st
    finally:
        s.close()


# ---- holding a side to the rules --------------------------------------------------------------------------------------------------------------------

def _key(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def compose_inputs(case, img):
    names = ("diffuse", "direct_raw") if case["lean"] else ("diffuse", "direct", "indirect", "reflection", "refraction", "transparent")
    return {k: img[k] for k in names}


def run_compose(case, img, mutate=None, lean=None):
    return CR.compose(img, lean=case["lean"] if lean is None else lean, ambient=case["ambient"], mutate=mutate)


def separate_post(case):
    v = case["view"]
    return bool(v.get("resolution_scale", 1.0) != 1.0 or v.get("motion_blur", 0.0) > 0.0 or v.get("upscaler", 0) or case["viewport"] or case["scissor"])


def hold_compose(case, img, side, rules=None, same_launch=True, log=print):
    """OUTPUT_RGBA32F, and the back buffer of a frame without a separate post pass, against tests/compose_rule.py.  same_launch: one launch stored both images, so the
    back buffer is the conversion of the stored float32, byte for byte.  rules: a cache {input bytes: rule result}."""
    name = case["name"]
    rules = {} if rules is None else rules
    inputs = compose_inputs(case, img)
    key = _key(*inputs.values())
    if key not in rules:
        rules[key] = run_compose(case, inputs)
    rule = rules[key]
    counts = dict(rule["info"]["counts"])
    additive = sum((np.asarray(img[k])[..., :3] != 0.0).any(axis=-1) for k in ("reflection", "refraction", "transparent") if k in inputs)
    counts["unlit_with_additive"] = int((~rule["lit"] & (additive > 0)).sum()) if not case["lean"] else 0
    c = CR.compare(img["output"], None if separate_post(case) else img["final"], rule)
    held = rule["lit"].size
    row = ("compose_rule %-18s %-10s ratio=%.6f/%.6f held=%d bad=%d final_bad=%d final_not_output=%d two_candidates=%d (%.4f of held) counts %s"
           % (side, name, c["ratio"][0], c["ratio"][1], held, int(c["bad"].sum()), c["final_bad"], c["final_not_output"], c["two_candidates"], c["two_candidates"] / held,
              {k: v for k, v in counts.items() if v}))
    log(row)
    assert counts["not_unorm8"] == 0 and counts["not_covered"] == 0, (name, counts)
    assert counts["unlit_with_additive"] == 0, (name, counts)          # no hit contributed where DIFFUSE.a = 0: nothing was added either (see COMPOSE_MUTATION_CASE)
    assert int(c["bad"].sum()) == 0 and c["ratio"][0] < 1.0, (name, c["ratio"], int(c["bad"].sum()))
    assert c["final_bad"] == 0, (name, c["final_bad"])
    assert not same_launch or c["final_not_output"] == 0, (name, c["final_not_output"])
    assert (np.asarray(img["output"])[..., 3] == 1.0).all()
    for k in REACH[name]:
        assert counts.get(k, 0) > 0, (name, k, counts)
    return row


def post_inputs(case, img):
    return dict(source=img[case["source"]], flow=img["flow"], before=img["background"] if case["background"] else None)


def run_post(case, img, mutate=None):
    i = post_inputs(case, img)
    out = np.asarray(img["output"])
    return PR.post_process(i["source"], i["flow"], case["size"], (out.shape[1], out.shape[0]), case["view"].get("motion_blur", 0.0), case["motion_blur_samples"],
                           viewport=case["viewport"], scissor=case["scissor"], before=i["before"], mutate=mutate)


def hold_post(case, img, side, rules=None, log=print):
    """FINAL_RGBA8 against tests/post_rule.py: inside the rectangles within the rule's interval, outside them the bytes the frame had before the pass."""
    name = case["name"]
    rules = {} if rules is None else rules
    i = post_inputs(case, img)
    key = _key(i["source"], i["flow"], *(() if i["before"] is None else (i["before"],)))
    if key not in rules:
        rules[key] = run_post(case, img)
    rule = rules[key]
    counts = rule["info"]["counts"]
    out, final = np.asarray(img["output"]), np.asarray(img["final"])
    assert final.shape == (case["size"][1], case["size"][0], 4) and (case["render"] is None or (out.shape[1], out.shape[0]) == case["render"]), (name, final.shape, out.shape)
    w, h = case["size"]
    assert np.asarray(i["source"]).shape[:2] == ((h, w) if case["source"] != "output" else out.shape[:2])
    c = PR.compare(final, rule)
    widest = float((rule["bound"][rule["inside"] & rule["covered"]] * 255.0).max()) if counts["inside"] else 0.0         # the largest bound, in RGBA8 steps
    row = ("post_rule %-18s %-15s ratio=%.6f/%.6f widest_bound=%.2e steps inside=%d bad=%d outside_bad=%d two_candidates=%d (%.4f of held) counts %s"
           % (side, name, c["ratio"][0], c["ratio"][1], widest, counts["inside"], c["bad"], c["outside_bad"], counts["two_candidates"],
              counts["two_candidates"] / max(counts["inside"], 1), {k: v for k, v in counts.items() if v and k not in ("inside", "two_candidates")}))
    log(row)
    assert counts["not_covered"] == 0, (name, counts["not_covered"])
    assert c["bad"] == 0 and c["ratio"][0] < 1.0, (name, c["bad"], c["ratio"])
    assert c["outside_bad"] == 0, (name, c["outside_bad"])
    for k in REACH[name]:
        assert counts.get(k, 0) > 0, (name, k, counts)
    if name == "blur":
        assert 2 * counts["blurred"] > w * h, (name, counts["blurred"])
    if name == "blur-still":
        assert counts["blurred"] == 0 and counts["near_threshold"] == 0 and (np.asarray(img["flow"]) == 0.0).all(), (name, counts)
    if not (case["viewport"] or case["scissor"]):
        assert counts["outside_rectangle"] == 0
    return row
