"""Scene cases of the GI-bounce rule tests (tests/test_gi_rule.py on the CPU oracle, tests/test_gpu_gi_rule.py on the GPU), the sessions both draw, and `hold`, which
compares INDIRECT_LIGHT_RAW, INDIRECT_LIGHT_FILTERED and GI_MOMENTS of every compared frame with tests/gi_rule.py.

Variants of the sample scene at 88 x 72 (wider than the 64-texel blue-noise tile: the modulo is exercised; no multiple of the 16-pixel tile) built on mirror_cases._base:
no normal or specular maps, colours k / 255 from diffuseColorMix.  A case is one session of two frames (three for `background`) drawn with max_reflections = 0 and the denoiser OFF, so that
giReproject = 0 and the rule needs no history; the slices move from frame to frame and frameCount + 64 wraps in the table.  The rule's inputs are the stored
SHADING_POSITION, SHADING_NORMAL and INSTANCE_ID (and IMAGE_BACKGROUND), and the scene.

Material alphas are 0.4 and 0.6, never 0.5: 0.5 * 255 = 127.5 is a UNORM8 tie."""
import numpy as np

import gi_rule as G
import light_cases as LC
import light_rule
import mirror_cases as MC
import primary_cases as PC

W, H = LC.W, LC.H
UNDECIDED_CAP = MC.UNDECIDED_CAP

CASES = ("opaque-1", "opaque-2", "opaque-3", "opaque-4", "self-lit", "layers", "background", "sky-strength", "two-bounce-opaque", "two-bounce-layers")

# Minimum ray counts that make a case worth running, asserted on the rule's own info over the compared frames: half of what the rule counts in the CPU run of the
# oracle (profiles/gi_rule_deviation.txt records the counts).  hit / miss: rays with and without an entry in their hit list; lit / shadowed: resolved surfaces whose
# drawn light reaches them / is occluded; two_contributing: hit lists with two or more contributing entries; sky: rays whose sky term is not zero.
SHARES = {
    "opaque-1": dict(hit=779, miss=2699, lit=643, shadowed=136),
    "opaque-2": dict(hit=1555, miss=5401, lit=1300, shadowed=254),
    "opaque-3": dict(hit=2344, miss=8089, lit=2009, shadowed=335),
    "opaque-4": dict(hit=1527, miss=5428, lit=1299, shadowed=228),
    "self-lit": dict(hit=443, miss=1845, lit=192, shadowed=52),
    "layers": dict(hit=2860, miss=2903, lit=2651, shadowed=209, two_contributing=615),
    "background": dict(hit=494, miss=2474, lit=467, sky=2474),
    "sky-strength": dict(hit=779, miss=2699, lit=643, shadowed=136, sky=2699),
    "two-bounce-opaque": dict(hit=964, miss=3275, lit=801, shadowed=162),
    "two-bounce-layers": dict(hit=2233, miss=2071, lit=2079, shadowed=154, two_contributing=590),
}

# the case built to catch each wrong variant of the rule.  (With one sample the slices frameCount + 64 and frameCount + 0 are the same slice: the variants that move the
# light pick to the sample's slice need two.  With 1, 2 or 4 samples the slices s * mult and (s - 1) * mult, s = n .. 1, are the same SET mod 64 and the mean of the
# samples does not see their order: `opaque-3`, mult = 21, slices 63, 42, 21 against 42, 21, 0, is the case that tells them apart.)
MUTATION_CASE = {
    "slice_from_zero": "opaque-3", "bn_no_xmod": "opaque-1", "uniform_weighting": "opaque-1", "tangent_swapped": "opaque-1", "no_depth_bias": "layers",
    "light_view_from_eye": "opaque-1", "no_shadow_ray": "opaque-1", "no_self_light": "self-lit", "no_gi_in_base": "opaque-1", "incoming_without_no_gi": "opaque-1",
    "albedo_unweighted": "layers", "sky_unweighted": "sky-strength", "diffuse_strength_on_sky": "sky-strength", "pick_per_sample": "opaque-2",
    "second_from_first_origin": "two-bounce-opaque", "second_on_first_slice": "two-bounce-opaque", "moments_of_mean": "opaque-2", "state_first_hit": "layers",
}

GPU_IMAGES = {"position": "SHADING_POSITION", "normal": "SHADING_NORMAL", "id": "INSTANCE_ID", "raw": "INDIRECT_LIGHT_RAW", "filtered": "INDIRECT_LIGHT_FILTERED",
              "moments": "GI_MOMENTS"}
ORACLE_IMAGES = {"position": "shadingPosition", "normal": "shadingNormal", "id": "instanceId", "raw": "indirectLight", "filtered": "filteredIndirect", "moments": "moments"}
INPUTS = ("position", "normal", "id", "background")


def _scene_lights(sample_data):
    stock = sample_data.lights[0]
    far = LC._light(stock, (15000.0, 30000.0, 15000.0), (0.8, 0.75, 0.65), radius=1e9, exponent=1.0, point_radius=5000.0)
    near = LC._light(stock, (-6.0, 4.0, 3.0), (0.9, 0.2, 0.1))
    side = LC._light(stock, (5.0, 3.0, 6.0), (0.1, 0.3, 0.9))
    return far, near, side


def make_case(sample_data, name):
    """dict(name, frames, compared, view (view description), bounces, background, data_at: frame -> SceneData)."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    d, sphere, floor = MC._base(sample_data)
    floor.material.reflectionFactor = 0.0
    V3 = type(sphere.material.selfLight)
    far, near, side = _scene_lights(sample_data)
    d.lights = [far, near, side]
    for i in (sphere, floor):                                         # a specular term that sees which way the view vector points
        i.material.specularExponent = 8.0
    case = dict(name=name, frames=2, compared=(0, 1), view=dict(di_samples=0, gi_samples=1, max_lights=12), bounces=1, background=False)

    def opaque():
        # floor, sphere, a wall behind them (it reaches below the floor's plane: a ray that leaves along the floor meets it squarely, not at its edge), an occluder over the floor between the near light and the ground
        w = MC._add_quad(d, "wall", (-3.0, 1.5, -4.0), 5.0, 2.0, "camera"); w.material.specularExponent = 8.0
        LC._add_quad(d, (-3.0, 1.5, 2.0), half=1.0).material.diffuseColorMix = type(floor.material.diffuseColorMix)(0.2, 0.4, 0.8, 1.0)
        return w

    def layers():
        # a wall with a light of its own; in front of it pane A (alpha 0.4) and, a quarter BEHIND A, pane C (alpha 0.6) whose depth bias of a half sorts it first;
        # C is taller than A and the wall: a ray through its upper part has C as its only, and last, contributing hit and goes on into the open
        w = MC._add_quad(d, "wall", (0.0, 1.5, -4.0), 7.0, 2.0, "camera"); w.material.selfLight = V3(0.1, 0.2, 0.05); MC._colour(w, (0, 153, 51))
        a = MC._add_quad(d, "paneA", (0.0, 1.5, -3.0), 7.0, 2.0, "camera"); a.material.solidAlphaMultiplier = 0.4
        c = MC._add_quad(d, "paneC", (0.0, 2.5, -3.25), 7.0, 3.0, "camera"); c.material.solidAlphaMultiplier = 0.6; c.material.depthBias = 0.5; MC._colour(c, (255, 204, 0))
        # the same pair as a canopy over the left of the floor, seen from below: most rays that leave the floor under it pass both, the steep ones (d.y > 1 / 2) the
        # upper, biased one first; nothing lies above them
        a = MC._add_quad(d, "canopyA", (-4.0, 4.5, 2.0), 3.0, 3.0, "down"); a.material.solidAlphaMultiplier = 0.4
        c = MC._add_quad(d, "canopyC", (-4.0, 4.75, 2.0), 4.0, 4.0, "down"); c.material.solidAlphaMultiplier = 0.6; c.material.depthBias = 0.5; MC._colour(c, (255, 204, 0))
        for i in d.instances:                                         # a translucent surface would let part of a shadow ray through: the panes cast no shadow at all
            if i.material.solidAlphaMultiplier != 1.0:
                i.material.shadowAlphaMultiplier = 0.0

    if name in ("opaque-1", "opaque-2", "opaque-3", "opaque-4"):
        opaque(); case["view"]["gi_samples"] = int(name.split("-")[1])
    elif name == "self-lit":
        # the wall shines by itself and its mask lets only the far light in; the sphere takes none of the lights
        w = opaque(); w.material.selfLight = V3(0.25, 0.125, 0.0); w.material.lightGroupMaskBits = 1
        sphere.material.lightGroupMaskBits = 0; sphere.material.selfLight = V3(0.0, 0.125, 0.25)
        d.lights = [LC._light(sample_data.lights[0], (15000.0, 30000.0, 15000.0), (0.8, 0.75, 0.65), radius=1e9, exponent=1.0, bits=1),
                    LC._light(sample_data.lights[0], (-6.0, 4.0, 3.0), (0.9, 0.2, 0.1), bits=2), LC._light(sample_data.lights[0], (5.0, 3.0, 6.0), (0.1, 0.3, 0.9), bits=3)]
    elif name == "layers":
        layers()
    elif name == "background":
        case["background"] = True; case["frames"] = 3; case["compared"] = (1, 2)
        PC._add_background(d, sample_data)
    elif name == "sky-strength":
        opaque()
        texels = np.tile(np.array([102, 153, 204, 255], dtype=np.uint8), (4, 4, 1))
        d.textures.append(sample_scene.TextureData("flat-sky", rt64.TEXTURE_FORMAT_RGBA8, texels, 4, 4)); d.sky = len(d.textures) - 1
        d.desc.skyDiffuseMultiplier = type(d.desc.skyDiffuseMultiplier)(0.5, 0.75, 1.25)
        d.desc.giSkyStrength = 0.5; d.desc.giDiffuseStrength = 1.25
        d.desc.ambientNoGIColor = type(d.desc.ambientNoGIColor)(0.05, 0.1, 0.15)
    elif name == "two-bounce-opaque":
        opaque(); case["bounces"] = 2; case["view"]["gi_samples"] = 2; case["compared"] = (1,)
    elif name == "two-bounce-layers":
        layers(); case["bounces"] = 2; case["compared"] = (1,)
    else:
        raise KeyError(name)
    if name == "opaque-4":
        case["compared"] = (1,)
    case["data_at"] = lambda frame: d
    return case


# ---- what the rule reads ----------------------------------------------------------------------------------------------------------------------------

def rule_scene(case, frame, background):
    from sm64rt_legacy_renderer_amd import rt64
    data = case["data_at"](frame)
    described = bool(case.get("sky_described"))                       # the cases of tests/sky_cases.py: `sky` is a description for tests/sky_rule.py
    scene = MC.rule_scene(data, case["view"], frame, sky_described=described)
    rt =[i for i in data.instances if data.meshes[i.mesh].flags & rt64.MESH_RAYTRACE_ENABLED]
    assert all(i.material.shadowAlphaMultiplier == (1.0 if i.material.solidAlphaMultiplier == 1.0 else 0.0) for i in rt)      # a shadow ray is stopped by an instance, or passes it freely
    scene["shadow"] = light_rule.BruteForceShadows([I["triangles"] for I, i in zip(scene["instances"], rt) if i.material.shadowAlphaMultiplier == 1.0])
    assert (background is not None) == case["background"]
    assert described or not (case["background"] and data.sky is not None), "a constant sky term or a background image, not both"
    e = data.desc
    cam = LC.rule_inputs(data)["camera"]
    scene.update(giSamples=int(case["view"]["gi_samples"]), giBounces=int(case["bounces"]), giDiffuseStrength=float(e.giDiffuseStrength), giSkyStrength=float(e.giSkyStrength),
                 skyAlpha=1.0 if data.sky is not None else 0.0, background=background, eye=np.linalg.inv(cam["view"])[3, :3])
    return scene


def run_rule(case, frame, img, mutate=None):
    """The rule for one compared frame on a side's stored images of that frame."""
    return G.indirect(rule_scene(case, frame, img["background"]), img["position"], img["normal"], img["id"], mutate=mutate)


# ---- sessions ---------------------------------------------------------------------------------------------------------------------------------------

def oracle_session(case):
    """{frame: images} of the CPU oracle for the compared frames."""
    from oracle import oracle_py
    out = {}
    o = oracle_py.OracleScene(case["data_at"](0))
    try:
        for f in range(case["frames"]):
            o.data = case["data_at"](f)
            ref = o.render(W, H, images=f in case["compared"], diSamples=case["view"]["di_samples"], giSamples=case["view"]["gi_samples"],
                           maxLights=case["view"]["max_lights"], maxReflections=0, giBounces=case["bounces"], denoiserEnabled=0)
            if f in case["compared"]:
                assert ref["pixelJitter"] == (0.0, 0.0)
                out[f] = {key: ref[name] for key, name in ORACLE_IMAGES.items()}
                out[f]["background"] = ref["background"] if case["background"] else None
    finally:
        o.close()
    return out


def gpu_session(rt64_lib, case, options=None, stats=None):
    """The same session on the device, with device options (a kernel path).  stats: a dict that receives {frame: FRAME_STATS}."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    out = {}
    s = sample_scene.Rt64Scene(rt64_lib, case["data_at"](0), W, H, hip_device=0)
    try:
        s.set_view_description(denoiser=False, **case["view"])
        assert s.option("max_reflections", 0) and s.option("gi_bounces", case["bounces"])
        for key, v in (options or {}).items():
            assert s.option(key, v), key
        for f in range(case["frames"]):
            s.data = case["data_at"](f)
            s.draw()
            if f in case["compared"]:
                if stats is not None:
                    stats[f] = s.stats()
                out[f] = {key: s.readback(getattr(rt64, "IMAGE_" + name)) for key, name in GPU_IMAGES.items()}
                out[f]["background"] = s.readback(rt64.IMAGE_BACKGROUND) if case["background"] else None
    finally:
        s.close()
    return out


# ---- holding a side to the rule ---------------------------------------------------------------------------------------------------------------------

def inputs_equal(a, b):
    return all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in INPUTS)


def judge(rule, img):
    """One frame's stored images against the rule: dict(ratio, mean, bad (pixels outside), undecided, surface)."""
    worst, mean, bad = G.compare(img["raw"], img["moments"], rule)
    return dict(ratio=worst, mean=mean, bad=int(bad.sum()), undecided=int((~rule["decided"]).sum()), surface=int(rule["surface"].sum()))


def hold(case, images, side, rules=None, log=print):
    """Every compared frame of a session against the rule; asserts the conditions of the tests and returns the report rows.  rules: a cache {frame: [(inputs, rule result)]}
    filled here: the rule runs once per (case, frame), and a kernel path whose stored inputs are the same bytes reuses the result."""
    rules = {} if rules is None else rules
    name = case["name"]
    rows, total = [], {}
    for f in case["compared"]:
        img = images[f]
        known = [r for i, r in rules.setdefault(f, []) if inputs_equal(i, img)]
        if not known:
            rules[f].append(({k: img[k] for k in INPUTS}, run_rule(case, f, img)))
            known = [rules[f][-1][1]]
        rule = known[0]
        # the writeFiltered copy: without a denoiser the filtered image is the raw one, byte for byte
        assert np.asarray(img["filtered"]).tobytes() == np.asarray(img["raw"]).tobytes(), (name, f, "INDIRECT_LIGHT_FILTERED is not INDIRECT_LIGHT_RAW")
        j = judge(rule, img)
        rows.append("gi_rule %-22s %-18s frame %d ratio=%.6f mean=%.6f surface=%d undecided=%d counts %s"
                    % (side, name, f, j["ratio"], j["mean"], j["surface"], j["undecided"], rule["info"]["counts"]))
        log(rows[-1])
        assert j["bad"] == 0 and j["ratio"] < 1.0, (name, f, j)
        assert j["undecided"] <= int(UNDECIDED_CAP * j["surface"]), (name, f, j["undecided"], j["surface"])
        for k, v in rule["info"]["counts"].items():
            total[k] = total.get(k, 0) + v
    for k, need in SHARES[name].items():
        assert total.get(k, 0) >= need and total.get(k, 0) > 0, (name, k, total.get(k, 0), need)
    return rows
