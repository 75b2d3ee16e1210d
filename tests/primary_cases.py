"""Scene cases of the primary-resolve rule tests (tests/test_primary_rule.py on the CPU oracle, tests/test_gpu_primary_rule.py on the GPU), the frame sequences
both draw, and `hold`, which compares every stored image of every compared frame with tests/primary_rule.py.

Variants of the sample scene at 88 x 72 built on mirror_cases._base (no sky, no background instance, no normal or specular maps, colours from diffuseColorMix).  A case
is one session of `frames` frames drawn with max_reflections = 0, so that no pass rewrites INSTANCE_ID or REFLECTION; each frame has its own camera, instance
transforms (transform and previousTransform as the host sends them) and canReproject flag.  The rule's inputs are the scene and the cameras, never a stored image.

Material alphas are 0.4 and 0.6, never 0.5: 0.5 * 255 = 127.5 is a UNORM8 tie."""
import copy

import numpy as np

import light_cases as LC
import light_rule
import mirror_cases as MC
import primary_rule as P

W, H = LC.W, LC.H
UNDECIDED_CAP = MC.UNDECIDED_CAP

CASES = ("static", "camera", "movers", "cut", "layers", "translucent-lit", "translucent-lit-2", "mirror-glass", "fog", "background", "jittered", "textured")

# Minimum pixel counts that make a case worth running, asserted on the rule's own info over the compared frames: half of what the rule counts in the CPU run
# of the oracle (profiles/primary_rule_deviation.txt records the counts).
SHARES = {
    "static": dict(hit=1772, miss=1394, still_hit=1772),
    "camera": dict(moving_hit=3176, moving_miss=2884),
    "movers": dict(moving_hit=1971, still_hit=2496),
    "cut": dict(moving_hit=992, moving_miss=1758, still_hit=1418),
    "layers": dict(two_contributing=661, later_store=274, behind_first=274, covered_no_hit=296),
    "translucent-lit": dict(two_contributing=937, transparent_light=1146, transparent_light_shadowed=138),
    "translucent-lit-2": dict(two_contributing=937, transparent_light=1146, transparent_light_shadowed=148),
    "mirror-glass": dict(two_mirrors=207, glass=594, lock_on=1515, lock_off=1134),
    "fog": dict(fog=1046, two_contributing=77, reactive_saturated=21),
    "background": dict(background=1683, covered_no_hit=387),
    "jittered": dict(moving_hit=4351, moving_miss=4380, lock_on=2507, lock_off=3147, background=5776),
    "textured": dict(textured=889),
}

# the case built to catch each wrong variant of the rule
MUTATION_CASE = {
    "state_last_hit": "layers", "state_from_unlit": "layers", "flow_x_not_negated": "camera", "flow_ignores_previous_transform": "movers",
    "flow_prev_matrix_current": "camera", "flow_not_in_pixels": "camera", "flow_miss_is_zero": "camera", "reproject_flag_ignored": "cut",
    "depth_without_bias": "layers", "fog_from_origin": "fog", "fresnel_direction_normalised": "mirror-glass", "reflect_alpha_summed": "mirror-glass",
    "lock_without_mirror_term": "mirror-glass", "lock_binary_with_upscaler": "jittered", "reactive_unclamped": "fog", "reactive_from_sum": "fog",
    "glass_keeps_coverage": "mirror-glass", "transparent_light_per_hit": "translucent-lit", "transparent_light_unshadowed": "translucent-lit",
    "background_uv_at_pixel_centre": "background", "jitter_not_in_uv": "jittered",
    "alpha_is_remaining_coverage": "layers", "order_by_t": "layers",
}

GPU_IMAGES = {"position": "SHADING_POSITION", "normal": "SHADING_NORMAL", "specular": "SHADING_SPECULAR", "diffuse": "DIFFUSE", "id": "INSTANCE_ID",
              "first_id": "FIRST_INSTANCE_ID", "transparent": "TRANSPARENT", "flow": "FLOW", "reactive": "REACTIVE_MASK", "lock": "LOCK_MASK", "depth": "DEPTH",
              "view": "VIEW_DIRECTION", "reflection": "REFLECTION", "refraction": "REFRACTION", "primary": "PRIMARY_HIT"}
ORACLE_IMAGES = {"position": "shadingPosition", "normal": "shadingNormal", "specular": "shadingSpecular", "diffuse": "diffuse", "id": "instanceId",
                 "transparent": "transparent", "flow": "flow", "reactive": "reactiveMask", "lock": "lockMask", "depth": "depth", "view": "viewDirection",
                 "reflection": "reflection", "refraction": "refraction", "primary": "primaryHit"}
UPSCALER_FSR, UPSCALER_MODE_NATIVE = 3, 6            # rt64.UPSCALER_FSR, rt64.UPSCALER_MODE_NATIVE


def _view(eye, yaw):
    """World -> view, row vectors: the camera at `eye`, turned by `yaw` about the vertical (float32 entries)."""
    c, s = np.float32(np.cos(yaw)), np.float32(np.sin(yaw))
    r = np.eye(4, dtype=np.float32); r[0, 0] = c; r[0, 2] = s; r[2, 0] = -s; r[2, 2] = c
    t = np.eye(4, dtype=np.float32); t[3, :3] = -np.asarray(eye, dtype=np.float32)
    return (t.astype(np.float64) @ r.astype(np.float64)).astype(np.float32)


def _turned(centre, angle):
    """Object -> world of a quad turned by `angle` about its vertical axis, then moved to `centre`."""
    c, s = np.float32(np.cos(angle)), np.float32(np.sin(angle))
    m = np.eye(4, dtype=np.float32); m[0, 0] = c; m[0, 2] = -s; m[2, 0] = s; m[2, 2] = c; m[3, :3] = centre
    return m


def _add_background(d, sample_data):
    """A raster background instance that covers the screen with a 64 x 64 texture whose channels rise by 8, 8 and 4 a texel (and wrap)."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    y, x = np.mgrid[0:64, 0:64]
    texels = np.stack([(8 * x) % 256, (8 * y) % 256, (4 * (x + y)) % 256, np.full_like(x, 255)], axis=-1).astype(np.uint8)
    d.textures.append(sample_scene.TextureData("gradient", rt64.TEXTURE_FORMAT_RGBA8, np.ascontiguousarray(texels), 64, 64))
    hud = next(i for i in sample_data.instances if i.flags & rt64.INSTANCE_RASTER_BACKGROUND)
    m = copy.copy(sample_data.meshes[hud.mesh]); v = m.vertices.copy()
    v["position"][:, :2] = [(-1.0, -1.0), (3.0, -1.0), (-1.0, 3.0)]; v["uv"] = [(0.0, 1.0), (2.0, 1.0), (0.0, -1.0)]
    m.vertices = v; d.meshes.append(m)
    b = copy.copy(hud); b.name = "backdrop"; b.mesh = len(d.meshes) - 1; b.diffuse = len(d.textures) - 1; b.material = sample_scene.copy_material(hud.material)
    d.instances.append(b)                          # last: the ids of the ray-traced instances stay what they were


def _moved(inst, transform, previous):
    c = copy.copy(inst); c.transform = transform; c.previous_transform = previous
    return c


def make_case(sample_data, name):
    """dict(name, frames, compared, view, upscaler, data_at: frame -> SceneData (its view is that frame's camera), reproject_at: frame -> canReproject)."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    d, sphere, floor = MC._base(sample_data)
    floor.material.reflectionFactor = 0.0
    stock = sample_data.lights[0]
    V3 = type(sphere.material.selfLight)
    case = dict(name=name, view=dict(di_samples=0, max_lights=12), frames=1, compared=(0,), upscaler=False, background=False)
    views, insts, reproject = None, None, {}
    eye = (0.0, 2.0, 10.0)
    strafe = [_view(eye, 0.0), _view((0.5, 2.0, 10.0), 0.03125), _view((1.25, 2.25, 9.5), 0.09375), _view((1.5, 2.25, 9.5), 0.125)]
    if name == "static":
        MC._add_quad(d, "wall", (-5.0, 2.0, -4.0), 3.0, 2.0, "camera")
    elif name in ("camera", "jittered"):
        MC._add_quad(d, "wall", (-5.0, 2.0, -4.0), 3.0, 2.0, "camera")
        views = strafe[:3] if name == "camera" else strafe
        case["frames"] = len(views); case["compared"] = (1, 2) if name == "camera" else (0, 1, 2, 3)
        if name == "jittered":
            case["upscaler"] = True; case["background"] = True
            floor.material.lockMask = 0.25; sphere.material.lockMask = 0.75
            _add_background(d, sample_data)
    elif name == "movers":
        q = MC._add_quad(d, "spinner", (-4.0, 2.0, 2.0), 1.5, 1.5, "camera"); q.flags |= rt64.INSTANCE_DISABLE_BACKFACE_CULLING
        ks, kq = d.instances.index(sphere), d.instances.index(q)
        def at(f):
            t = np.eye(4, dtype=np.float32); t[3, 0] = 0.25 * f
            return t, _turned((-4.0, 2.0, 2.0), 0.125 * f)
        seq = {}
        for f in range(4):
            cur = at(min(f, 2)); prev = at(max(min(f, 3) - 1, 0))          # frame 3: both have stopped at frame 2's place, previousTransform is still frame 1's
            if f == 3:
                prev = at(1)
            l = list(d.instances); l[ks] = _moved(sphere, cur[0], prev[0]); l[kq] = _moved(q, cur[1], prev[1])
            seq[f] = l
        insts = seq; d.instances = seq[0]
        case["frames"] = 4; case["compared"] = (1, 2, 3)
    elif name == "cut":
        MC._add_quad(d, "wall", (-5.0, 2.0, -4.0), 3.0, 2.0, "camera")
        views = [strafe[0], _view((3.0, 3.0, 9.0), 0.25), _view((3.25, 3.0, 9.0), 0.28125)]
        reproject = {1: False}
        case["frames"] = 3; case["compared"] = (1, 2)
    elif name == "layers":
        # A: lit, alpha 0.6, at t = 6.  C: lit, alpha 0.6, a quarter BEHIND A with a depth bias of a half, so sorted first by t - depthBias only; it overlaps A's left half.
        # B: mask 0 and alpha 0.4 in front of sphere and floor: stores nothing.  D: mask 0, alone against the sky.
        a = MC._add_quad(d, "paneA", (-1.5, 1.5, 4.0), 1.0, 1.0, "camera"); a.material.solidAlphaMultiplier = 0.6
        c = MC._add_quad(d, "paneC", (-2.25, 1.5, 3.75), 0.75, 0.75, "camera"); c.material.solidAlphaMultiplier = 0.6; c.material.depthBias = 0.5; MC._colour(c, (255, 204, 0))
        b = MC._add_quad(d, "paneB", (1.5, 1.5, 4.0), 1.0, 1.0, "camera"); b.material.solidAlphaMultiplier = 0.4; b.material.lightGroupMaskBits = 0
        b.material.selfLight = V3(0.25, 0.125, 0.0); MC._colour(b, (0, 153, 51))
        e = MC._add_quad(d, "paneD", (3.0, 6.5, -4.0), 2.0, 1.0, "camera"); e.material.solidAlphaMultiplier = 0.6; e.material.lightGroupMaskBits = 0
    elif name in ("translucent-lit", "translucent-lit-2"):
        # two lit panes at alpha 0.4, one behind the other (the second larger), three lights, an opaque occluder between the near light and part of the first pane
        far = LC._light(stock, (15000.0, 30000.0, 15000.0), (0.8, 0.75, 0.65), radius=1e9, exponent=1.0, point_radius=5000.0)
        near = LC._light(stock, (-6.0, 4.0, 8.0), (0.9, 0.2, 0.1), point_radius=0.5)
        side = LC._light(stock, (5.0, 3.0, 9.0), (0.1, 0.3, 0.9), point_radius=0.5)
        d.lights = [far, near, side]
        case["view"] = dict(di_samples=2 if name.endswith("-2") else 0, max_lights=12)
        a = MC._add_quad(d, "first", (-1.0, 1.5, 4.0), 1.5, 1.0, "camera"); a.material.solidAlphaMultiplier = 0.4; a.material.shadowAlphaMultiplier = 0.0
        b = MC._add_quad(d, "second", (-0.5, 1.5, 3.0), 2.5, 1.5, "camera"); b.material.solidAlphaMultiplier = 0.4; b.material.shadowAlphaMultiplier = 0.0
        MC._colour(b, (255, 204, 0))
        MC._add_quad(d, "occluder", (-3.0, 2.5, 6.0), 0.75, 0.75, "camera").flags |= rt64.INSTANCE_DISABLE_BACKFACE_CULLING
    elif name == "mirror-glass":
        floor.material.reflectionFactor = 0.3; floor.material.reflectionFresnelFactor = 0.5
        p = MC._add_quad(d, "pane", (-2.0, 1.0, 4.0), 1.0, 1.0, "camera"); p.material.solidAlphaMultiplier = 0.6
        p.material.reflectionFactor = 0.5; p.material.reflectionFresnelFactor = 1.5; p.material.lockMask = 0.3
        sphere.material.refractionFactor = 0.9; sphere.material.solidAlphaMultiplier = 0.6; sphere.material.lockMask = 0.3
        wl = MC._add_quad(d, "wall", (0.0, 3.0, -4.0), 7.0, 3.0, "camera"); wl.material.lockMask = 0.7; MC._colour(wl, (0, 153, 51))
    elif name == "fog":
        floor.material.fogEnabled = 1; floor.material.fogMul = 4000.0; floor.material.fogOffset = -3720.0; floor.material.fogColor = V3(0.5, 0.75, 1.0)
        p = MC._add_quad(d, "pane", (3.5, 1.5, 2.0), 1.5, 1.0, "camera"); p.material.solidAlphaMultiplier = 0.6
        p.material.fogEnabled = 1; p.material.fogMul = 4000.0; p.material.fogOffset = -3720.0; p.material.fogColor = V3(1.0, 0.75, 0.5)
    elif name == "background":
        # the gradient shows whole where the ray misses and through two panes: an unlit one against it alone, a lit one over the floor's far edge
        case["background"] = True
        a = MC._add_quad(d, "high", (3.0, 6.5, -4.0), 2.0, 1.0, "camera"); a.material.solidAlphaMultiplier = 0.6; a.material.lightGroupMaskBits = 0
        b = MC._add_quad(d, "low", (-4.0, 4.5, -4.0), 2.0, 1.5, "camera"); b.material.solidAlphaMultiplier = 0.4
        _add_background(d, sample_data)
    elif name == "textured":
        # the floor takes its colour from a one-level RGBA8 texture (TEX0: diffuseColorMix.w = 0)
        floor.material.diffuseColorMix = type(floor.material.diffuseColorMix)(0.0, 0.0, 0.0, 0.0)
    else:
        raise KeyError(name)

    def data_at(frame):
        c = copy.copy(d)
        if views is not None:
            c.view = views[frame]
        if insts is not None:
            c.instances = insts[frame]
        return c
    case["data_at"] = data_at; case["reproject_at"] = lambda f: reproject.get(f, True)
    return case


# ---- what the rule reads -------------------------------------------------------------------------------------------------------------------------

def _camera(case, frame):
    d = case["data_at"](frame)
    w, h = _size(case)
    return dict(view=np.asarray(d.view, dtype=np.float32), fov=float(np.float32(d.fov)), near=float(np.float32(d.near)), far=float(np.float32(d.far)), width=w, height=h)


def _size(case):
    """88 x 72, but for the cases of tests/sky_cases.py that set a size of their own (the aspect ratio enters the sky plane's UV)."""
    return case.get("size", (W, H))


def rule_inputs(case, frame, background=None):
    from sm64rt_legacy_renderer_amd import rt64
    data = case["data_at"](frame)
    scene = MC.rule_scene(data, case["view"], frame, sky_described=bool(case.get("sky_described")))
    rt = [i for i in data.instances if data.meshes[i.mesh].flags & rt64.MESH_RAYTRACE_ENABLED]
    for I, inst in zip(scene["instances"], rt):
        mesh = data.meshes[inst.mesh]
        I["material"]["lockMask"] = float(inst.material.lockMask)
        I["previousTransform"] = np.asarray(inst.previous_transform, dtype=np.float32)
        I["object_triangles"] = mesh.vertices["position"].astype(np.float64)[:, :3][np.asarray(mesh.indices, dtype=np.int64)].reshape(-1, 3, 3)
        assert inst.material.shadowAlphaMultiplier in (0.0, 1.0)              # a shadow ray passes an instance freely, or is stopped by it
    # the casters of a shadow ray: the instances whose shadow alpha is 1 (the any-hit subtracts alpha x shadowAlphaMultiplier from the ray's visibility)
    scene["shadow"] = light_rule.BruteForceShadows([I["triangles"] for I, inst in zip(scene["instances"], rt) if inst.material.shadowAlphaMultiplier == 1.0])
    cam = _camera(case, frame)
    cam.update(frameCount=frame, canReproject=case["reproject_at"](frame), previous=_camera(case, frame - 1) if frame > 0 else None, upscaler=case["upscaler"],
               phases=P.phase_count(W, W), background=background)
    assert (background is not None) == case["background"]
    return scene, cam


def run_rule(case, frame, images, mutate=None):
    """The rule for one compared frame; `images` are a side's stored images of the session (only a case with a background instance reads one: BACKGROUND)."""
    scene, cam = rule_inputs(case, frame, images[frame]["background"] if case["background"] else None)
    return with_tables(P.primary(scene, cam, mutate=mutate), scene)


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------------

def _frames(case):
    now = None
    for f in range(case["frames"]):
        d = case["data_at"](f)
        changed = [] if now is None else [(j, inst) for j, inst in enumerate(d.instances) if inst is not now[j]]
        now = list(d.instances)
        yield f, d, changed


def oracle_session(case):
    """{frame: images} of the CPU oracle for the compared frames."""
    from oracle import oracle_py
    out = {}
    o = oracle_py.OracleScene(case["data_at"](0))
    try:
        up = dict(upscaler=UPSCALER_FSR, upscalerMode=UPSCALER_MODE_NATIVE) if case["upscaler"] else {}
        for f, d, changed in _frames(case):
            for j, inst in changed:
                o.set_instance(j, inst)
            o.data = d
            ref = o.render(*_size(case), images=f in case["compared"], can_reproject=case["reproject_at"](f), diSamples=case["view"]["di_samples"],
                           maxLights=case["view"]["max_lights"], maxReflections=0, **up)
            if f in case["compared"]:
                out[f] = {key: ref[name] for key, name in ORACLE_IMAGES.items()}
                out[f]["jitter"] = ref["pixelJitter"]; out[f]["background"] = ref["background"]
    finally:
        o.close()
    return out


def gpu_session(rt64_lib, case, options=None, view=None, stats=None):
    """The same session on the device, with device options (a kernel path) and view-description overrides.  stats: a dict that receives {frame: FRAME_STATS}."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    out = {}
    s = sample_scene.Rt64Scene(rt64_lib, case["data_at"](0), *_size(case), hip_device=0)
    try:
        up = dict(upscaler=UPSCALER_FSR, upscaler_mode=UPSCALER_MODE_NATIVE) if case["upscaler"] else {}
        s.set_view_description(**dict(case["view"], **dict(up, **(view or {}))))
        assert s.option("max_reflections", 0)
        for key, v in (options or {}).items():
            assert s.option(key, v), key
        for f, d, changed in _frames(case):
            for j, inst in changed:
                s.set_instance(j, inst)
            s.data = d
            s.draw(can_reproject=case["reproject_at"](f))
            if f in case["compared"]:
                if stats is not None:
                    stats[f] = s.stats()
                out[f] = {key: s.readback(getattr(rt64, "IMAGE_" + name)) for key, name in GPU_IMAGES.items()}
                out[f]["background"] = s.readback(rt64.IMAGE_BACKGROUND) if case["background"] else None
    finally:
        s.close()
    return out


# ---- holding a side to the rule ------------------------------------------------------------------------------------------------------------------

def _ratio(stored, value, bound):
    stored = np.asarray(stored, dtype=np.float64)
    if stored.ndim == 2:
        stored = stored[..., None]
    dev = np.abs(stored[..., :value.shape[-1]] - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dev == 0.0, 0.0, dev / bound)
    return np.where(np.isnan(r), np.inf, r).max(axis=-1)


def judge(rule, img):
    """One frame's stored images against the rule.  Returns dict(ratios {image: (largest, mean)}, bad (H, W) bool: a decided pixel outside the rule in any image)."""
    dec, lock_dec = rule["decided"], rule["lock_decided"]
    bad = np.zeros(dec.shape, dtype=bool)
    ratios = {}
    stored = {"reflection_a": np.asarray(img["reflection"])[..., 3:4], "refraction_a": np.asarray(img["refraction"])[..., 3:4]}
    for name in P.IMAGES:
        v, b = rule["images"][name]
        r = _ratio(stored.get(name, img.get(name)), v, b)
        ok = np.ones_like(dec) if name == "view" else (lock_dec if name == "lock" else dec)      # no decision touches the ray
        if name == "lock" and rule["lock_binary"]:
            r = np.where(np.asarray(img["lock"], dtype=np.float64) == v[..., 0], 0.0, np.inf)
        bad |= ok & (r >= 1.0)
        ratios[name] = (float(r[ok].max()), float(np.where(np.isfinite(r[ok]), r[ok], 1e9).mean()))
    # the ids and "has a stored hit": equal
    ids = np.asarray(img["id"]).astype(np.int64)
    wrong_id = dec & (ids != rule["id"])
    if "first_id" in img:
        wrong_id |= dec & (np.asarray(img["first_id"]).astype(np.int64) != rule["id"])
    bad |= wrong_id
    ratios["id"] = (float(wrong_id.sum()), 0.0)
    # DIFFUSE: the stored byte lies among the bytes the interval allows
    byte = np.rint(np.asarray(img["diffuse"], dtype=np.float64) * 255.0)
    off = dec & ((byte < rule["diffuse_lo"]) | (byte > rule["diffuse_hi"])).any(axis=-1)
    bad |= off
    ratios["diffuse"] = (float(off.sum()), float((rule["diffuse_hi"] - rule["diffuse_lo"])[dec].mean()))
    # REFLECTION.rgb = 0 (V14; with max_reflections = 0 no pass adds to it)
    lit = (np.asarray(img["reflection"])[..., :3] != 0).any(axis=-1)
    bad |= lit
    # (V3) the first list entry is the stored PRIMARY_HIT record
    first, rec = rule["first"], np.asarray(img["primary"]).astype(np.uint32)
    some = first["count"] > 0
    none_ok = (rec == 0xFFFFFFFF).all(axis=-1)
    tuv = np.ascontiguousarray(rec[..., :3]).view(np.float32).astype(np.float64)
    tri_inst, tri_prim = rule["tri_inst"], rule["tri_prim"]
    t = first["tri"].astype(np.int64)
    same = ((rec[..., 3] >> 24) == tri_inst[t]) & ((rec[..., 3] & 0xFFFFFF) == tri_prim[t])
    with np.errstate(invalid="ignore"):
        near = (np.abs(tuv[..., 0] - first["t"]) <= first["dt"] + light_rule.U * np.abs(first["t"])) & (np.abs(tuv[..., 1] - first["u"]) <= first["du"] + light_rule.U) \
            & (np.abs(tuv[..., 2] - first["v"]) <= first["dv"] + light_rule.U)
    wrong_hit = dec & np.where(some, ~(same & near), ~none_ok)
    bad |= wrong_hit
    ratios["primary_hit"] = (float(wrong_hit.sum()), 0.0)
    return dict(ratios=ratios, bad=bad)


def counts(rule):
    """What a case was built for, counted on the rule's own info (decided pixels)."""
    i, dec = rule["info"], rule["decided"]
    flow = np.abs(i["flow"]).max(axis=-1)
    first_inst = rule["tri_inst"][rule["first"]["tri"].astype(np.int64)]
    return dict(hit=int((dec & i["has_hit"]).sum()), miss=int((dec & (i["hits"] == 0)).sum()), moving_hit=int((dec & i["has_hit"] & (flow > 0.25)).sum()),
                moving_miss=int((dec & ~i["has_hit"] & (flow > 0.25)).sum()), still_hit=int((dec & i["has_hit"] & (flow == 0.0)).sum()),
                two_contributing=int((dec & (i["contributing"] >= 2)).sum()), later_store=int((dec & (i["storing_hit"] >= 1)).sum()),
                behind_first=int((dec & i["has_hit"] & (i["hits"] > 0) & (first_inst != rule["id"])).sum()),
                covered_no_hit=int((dec & ~i["has_hit"] & (i["coverage"] > 0.0)).sum()), two_mirrors=int((dec & (i["mirrors"] >= 2)).sum()), glass=int((dec & i["glass"]).sum()),
                lock_on=int((rule["lock_decided"] & (i["lock"] >= 0.5)).sum()), lock_off=int((rule["lock_decided"] & (i["lock"] > 0.0) & (i["lock"] < 0.5)).sum()),
                fog=int((dec & i["fog"]).sum()), textured=int((dec & i["textured"]).sum()), background=int((dec & i["background"]).sum()), reactive_saturated=int((dec & (i["reactive"] > 0.9)).sum()), transparent_light=int((dec & i["transparent_light"]).sum()), transparent_light_shadowed=int((dec & i["transparent_light_shadowed"]).sum()))


def with_tables(rule, scene):
    import mirror_rule
    _, _, _, inst, prim = mirror_rule.scene_triangles(scene)
    rule["tri_inst"], rule["tri_prim"] = inst, prim
    return rule


def rules_of(case, images, cache=None):
    """{frame: rule result} for the compared frames; computed once per case (the rule's inputs are the scene, not images -- but for BACKGROUND, whose bytes a
    cached result remembers and requires of every other set of images it is used for)."""
    cache = {} if cache is None else cache
    for f in case["compared"]:
        if f not in cache:
            cache[f] = run_rule(case, f, images)
            cache[f]["background"] = images[f]["background"]
        elif case["background"]:
            assert np.array_equal(cache[f]["background"], images[f]["background"]), ("BACKGROUND differs from the one the rule was computed with", f)
    return cache


def hold(case, images, side, rules=None, log=print):
    """Every image of every compared frame against the rule; asserts the conditions of the tests and returns the report rows."""
    rules = rules_of(case, images, rules)
    name = case["name"]
    rows, total = [], {}
    for f in case["compared"]:
        rule, img = rules[f], images[f]
        if "jitter" in img:
            assert np.allclose(img["jitter"], rule["info"]["jitter"], rtol=0, atol=1e-6), (img["jitter"], rule["info"]["jitter"])
        j = judge(rule, img)
        und = rule["info"]["undecided"]
        n_und = int((~rule["decided"]).sum())
        for image, (worst, mean) in j["ratios"].items():
            rows.append("primary_rule %-22s %-16s frame %d %-13s largest=%.6f mean=%.6f" % (side, name, f, image, worst, mean))
            log(rows[-1])
        rows.append("primary_rule %-22s %-16s frame %d undecided=%d %s" % (side, name, f, n_und, {x: y for x, y in und.items() if y}))
        log(rows[-1])
        assert int(j["bad"].sum()) == 0, (name, f, int(j["bad"].sum()), {k: v for k, v in j["ratios"].items() if v[0] >= 1.0})
        assert n_und + und["lock_step"] <= int(UNDECIDED_CAP * W * H), (name, f, n_und, und)
        for k, v in counts(rule).items():
            total[k] = total.get(k, 0) + v
    rows.append("primary_rule %-22s %-16s counts %s" % (side, name, {k: v for k, v in total.items() if v}))
    log(rows[-1])
    for k, need in SHARES.get(name, {}).items():
        assert total[k] >= need, (name, k, total[k], need)
    return rows
