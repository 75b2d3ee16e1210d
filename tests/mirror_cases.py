"""Scene cases of the mirror / glass rule tests (tests/test_mirror_rule.py on the CPU oracle, tests/test_gpu_mirror_rule.py on the GPU), and the session scheme both use.

Variants of the sample scene at 88 x 72 (as tests/light_cases.py: the blue-noise address wraps, the tiles are partial) without sky, background instance, normal and
specular maps; every surface takes its colour from diffuseColorMix (k / 255, w = 1) except the floor of `textured`, which keeps its texture.  Every coordinate added here is a small multiple of a power of two, so the
float64 world-space triangles are the float32 ones exactly.

The session scheme (a readback folds the reflection passes' continuation state into the G-buffer, so a pass's inputs cannot be read in the session that runs it):
session k draws the case with max_reflections = k.  Session 0 holds the pristine G-buffer and REFLECTION = (0, 0, 0, alpha); session k holds REFLECTION after k passes
and the folded state.  The rule for pass k takes session k's stored images and predicts session k + 1's.  Refraction runs once, before and independently of the
reflection passes: its inputs are session 0's images and its own alpha."""
import copy
import ctypes as C

import numpy as np

import light_cases as LC
import light_rule
import mirror_rule as M

W, H = LC.W, LC.H
UNDECIDED_CAP = 0.005

CASES = ("floor", "lights", "unlit", "facing", "lone-pixel", "lone-pixel-none", "translucent", "textured", "sky", "glass", "frames")

# Minimum shares that make a case worth running, asserted on the rule's own info (pass 0 unless said otherwise):
#   mirrored: pixels pass 0 takes; surface: share of them whose ray ends on a surface; on: share that goes on to pass 1
SHARES = {
    "floor": dict(mirrored=1500, surface=0.10), "lights": dict(mirrored=1500, surface=0.10), "unlit": dict(mirrored=1500, surface=0.15),
    "facing": dict(mirrored=2500, surface=0.25, on=0.10), "lone-pixel": dict(mirrored=1500, surface=0.10), "lone-pixel-none": dict(mirrored=1500, surface=0.10),
    "translucent": dict(mirrored=1500, surface=0.10, three=0.02), "textured": dict(mirrored=1500, surface=0.10, textured=0.05),
    "sky": dict(mirrored=1500, surface=0.10), "glass": dict(glass=500, total_internal=0.05), "frames": dict(mirrored=1500, surface=0.10),
}

# the case built to catch each wrong variant of the rule (tests/test_mirror_rule.py tries it first), and the pass it shows in
MUTATION_CASE = {
    "fresnel_from_hit": ("facing", 0), "fresnel_no_floor": ("facing", 0), "mirror_fog_from_camera": ("unlit", 0), "mirror_shadows": ("lights", 0),
    "glass_no_shadows": ("glass", 0), "eye_light": ("floor", 0), "direction_normalised": ("floor", 0), "k_unsaturated": ("facing", 0), "shine_abs": ("floor", 0),
    "state_without_hit": ("floor", 0), "state_first_hit": ("sky", 0), "state_lit_only": ("unlit", 0), "eta_inverted": ("glass", 0), "tir_ignored": ("glass", 0),
    "order_by_t": ("unlit", 0), "light_slot_plus_one": ("lights", 0), "no_flip": ("translucent", 0), "texel_point": ("textured", 0),
}

GPU_IMAGES = {"position": "SHADING_POSITION", "view": "VIEW_DIRECTION", "normal": "SHADING_NORMAL", "id": "INSTANCE_ID", "reflection": "REFLECTION",
              "refraction": "REFRACTION", "diffuse": "DIFFUSE", "direct": "DIRECT_LIGHT_RAW", "primary": "PRIMARY_HIT"}
ORACLE_IMAGES = {"position": "shadingPosition", "view": "viewDirection", "normal": "shadingNormal", "id": "instanceId", "reflection": "reflection",
                 "refraction": "refraction", "diffuse": "diffuse", "direct": "directLight", "primary": "primaryHit"}
STATE = ("position", "view", "normal", "id")
UNTOUCHED = ("diffuse", "direct", "primary")


def _colour(inst, rgb):
    inst.material.diffuseColorMix = type(inst.material.diffuseColorMix)(rgb[0] / 255.0, rgb[1] / 255.0, rgb[2] / 255.0, 1.0)


def _add_quad(d, name, centre, half_x, half_z, facing):
    """A quad of its own mesh and instance.  facing "down": horizontal, seen from below; "camera": vertical, in the xy plane, seen from +z; "up": horizontal, seen from above."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    floor = next(i for i in d.instances if i.name == "floor")
    v = d.meshes[floor.mesh].vertices[:4].copy()
    if facing == "camera":
        v["position"] = [(-half_x, -half_z, 0.0, 1.0), (half_x, -half_z, 0.0, 1.0), (-half_x, half_z, 0.0, 1.0), (half_x, half_z, 0.0, 1.0)]
        v["normal"] = (0.0, 0.0, 1.0); idx = [0, 1, 2, 3, 2, 1]
    else:
        v["position"] = [(-half_x, 0.0, -half_z, 1.0), (half_x, 0.0, -half_z, 1.0), (-half_x, 0.0, half_z, 1.0), (half_x, 0.0, half_z, 1.0)]
        v["normal"] = (0.0, 1.0, 0.0) if facing == "up" else (0.0, -1.0, 0.0)
        idx = [2, 1, 0, 1, 2, 3] if facing == "up" else [0, 1, 2, 3, 2, 1]
    d.meshes.append(sample_scene.MeshData(name, rt64.MESH_RAYTRACE_ENABLED, v, np.array(idx, dtype=np.uint32)))
    t = np.eye(4, dtype=np.float32); t[3, :3] = centre
    q = copy.copy(floor); q.name = name; q.mesh = len(d.meshes) - 1; q.transform = t; q.previous_transform = t
    q.material = sample_scene.base_material(); q.normal = None; q.specular = None
    _colour(q, (51, 102, 204))
    d.instances.append(q)
    return q


def _base(sample_data):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    d = copy.copy(sample_data)
    d.desc = type(sample_data.desc)(); C.memmove(C.byref(d.desc), C.byref(sample_data.desc), C.sizeof(d.desc))
    d.instances = [copy.copy(i) for i in sample_data.instances if not (i.flags & rt64.INSTANCE_RASTER_BACKGROUND)]      # background instances: out of scope
    for i in d.instances:
        i.material = sample_scene.copy_material(i.material); i.normal = None; i.specular = None
    d.meshes = list(sample_data.meshes); d.textures = list(sample_data.textures); d.lights = list(sample_data.lights)
    d.sky = None
    sphere = next(i for i in d.instances if i.name == "sphere"); floor = next(i for i in d.instances if i.name == "floor")
    _colour(sphere, (204, 51, 51)); _colour(floor, (153, 153, 102))
    floor.material.reflectionFactor = 0.3; floor.material.reflectionShineFactor = 0.2; floor.material.reflectionFresnelFactor = 0.5
    return d, sphere, floor


def _with(inst, **material):
    """A copy of an instance with material fields (and `transform`) replaced."""
    from sm64rt_legacy_renderer_amd import sample_scene
    c = copy.copy(inst); c.material = sample_scene.copy_material(inst.material)
    for k, v in material.items():
        if k == "transform":
            c.transform = v; c.previous_transform = v
        else:
            setattr(c.material, k, v)
    return c


def make_case(sample_data, name):
    """dict(data_at: frame -> SceneData, view: the view description, frames: frames drawn, compared: the frames compared, passes: reflection passes held to the rule,
    glass: the refraction pass is held to the rule)."""
    d, sphere, floor = _base(sample_data)
    stock = sample_data.lights[0]
    V3 = type(sphere.material.selfLight)
    far = LC._light(stock, (15000.0, 30000.0, 15000.0), (0.8, 0.75, 0.65), radius=1e9, exponent=1.0, point_radius=5000.0)
    near = LC._light(stock, (-6.0, 4.0, 3.0), (0.9, 0.2, 0.1), point_radius=0.5)
    below = LC._light(stock, (0.5, -3.0, -4.0), (0.3, 0.6, 0.3), point_radius=0.25)
    dim = LC._light(stock, (0.0, 6.0, 8.0), (0.0002, 0.0002, 0.0002))
    case = dict(view=dict(di_samples=0, max_lights=12), frames=1, compared=(0,), passes=2, glass=False)
    by_frame = None
    if name == "floor":
        pass
    elif name == "lights":
        d.lights = [far, near, below, dim]; case["view"] = dict(di_samples=2, max_lights=3)
        sphere.material.ignoreNormalFactor = 0.5; sphere.material.specularExponent = 8.0; sphere.material.selfLight = V3(0.05, 0.02, 0.0)
    elif name == "unlit":
        sphere.material.lightGroupMaskBits = 0; sphere.material.selfLight = V3(0.25, 0.125, 0.0)
        # a wall behind the sphere, foggy by its distance from the mirror; beside it an unlit pane a quarter in front of a second wall whose depth bias of a half
        # puts it first in the hit order although its t is larger (order by t - depthBias); that wall is opaque, so the pane contributes only if it is sorted first
        q = _add_quad(d, "wall", (-5.0, 2.0, -4.0), 3.0, 2.0, "camera")
        q.material.fogEnabled = 1; q.material.fogMul = 16.0; q.material.fogOffset = -2.0; q.material.fogColor = V3(0.5, 0.75, 1.0)
        p = _add_quad(d, "pane", (5.0, 2.0, -3.75), 3.0, 2.0, "camera"); _colour(p, (255, 204, 0))
        p.material.lightGroupMaskBits = 0
        b = _add_quad(d, "back", (5.0, 2.0, -4.0), 3.0, 2.0, "camera"); _colour(b, (0, 153, 51)); b.material.depthBias = 0.5
    elif name == "facing":
        sphere.material.reflectionFactor = 0.1; sphere.material.reflectionFresnelFactor = 2.0
        q = _add_quad(d, "ceiling", (6.0, 0.5, 1.0), 3.0, 5.0, "down")
        q.material.reflectionFactor = 0.5; q.material.reflectionFresnelFactor = 1.5; q.material.reflectionShineFactor = 0.5
        case["passes"] = 5
    elif name in ("lone-pixel", "lone-pixel-none", "frames"):
        q = _add_quad(d, "shard", (3.0, 0.5, 1.0), 0.25, 0.25, "down")
        q.material.reflectionFactor = 0.5; q.material.reflectionFresnelFactor = 1.5
        if name == "lone-pixel-none":
            q.material.reflectionFactor = 0.0
        if name == "frames":
            # the shard is in reach in frames 0, 1, 4 and 6, moved away in 2 and 3; frame 5 has no mirror at all: no pass is launched and no flag cleared
            k = d.instances.index(q)
            away = np.eye(4, dtype=np.float32); away[3, :3] = (3.0, 64.0, 1.0)
            moved = _with(q, transform=away)
            dull = [_with(i, reflectionFactor=0.0) for i in d.instances]
            here = list(d.instances)
            gone = list(d.instances); gone[k] = moved
            by_frame = {0: here, 1: here, 2: gone, 3: gone, 4: here, 5: dull, 6: here}
            case["frames"] = 7; case["compared"] = (1, 3, 4, 6); case["passes"] = 3
    elif name == "translucent":
        # the sphere keeps its back faces and is translucent: a mirror ray through it has two hits on it, the second on a back face whose normal is turned against the
        # ray; behind it two translucent panes, the farther one with a depth bias of a half that sorts it first although it lies a quarter behind the other.
        # (solidAlphaMultiplier 0.5 would be 127.5 / 255: a UNORM8 tie that float32 decides by u and v -- see DESIGN.md; 0.6 is 153 / 255.)
        from sm64rt_legacy_renderer_amd import rt64
        sphere.material.solidAlphaMultiplier = 0.6; sphere.flags |= rt64.INSTANCE_DISABLE_BACKFACE_CULLING
        sphere.material.reflectionFactor = 0.1; sphere.material.reflectionFresnelFactor = 2.0      # both of its hits enter the Fresnel sum with their normals
        p = _add_quad(d, "pane", (0.0, 2.0, -4.25), 7.0, 2.0, "camera"); p.material.solidAlphaMultiplier = 0.4; p.material.depthBias = 0.5
        b = _add_quad(d, "back", (0.0, 2.0, -4.0), 7.0, 2.0, "camera"); _colour(b, (0, 153, 51)); b.material.solidAlphaMultiplier = 0.8
    elif name == "textured":
        # the floor keeps its texture (diffuseColorMix.w = 0) and is seen in a mirror wall behind the sphere; it mirrors too, so those pixels go on
        floor.material.diffuseColorMix = type(floor.material.diffuseColorMix)(0.0, 0.0, 0.0, 0.0)
        q = _add_quad(d, "wall", (-5.0, 2.0, -4.0), 3.0, 2.0, "camera")
        q.material.reflectionFactor = 0.5; q.material.reflectionFresnelFactor = 1.5
    elif name == "sky":
        from sm64rt_legacy_renderer_amd import rt64, sample_scene
        texels = np.tile(np.array([102, 153, 204, 255], dtype=np.uint8), (4, 4, 1))
        d.textures.append(sample_scene.TextureData("flat-sky", rt64.TEXTURE_FORMAT_RGBA8, texels, 4, 4)); d.sky = len(d.textures) - 1
        d.desc.skyDiffuseMultiplier = type(d.desc.skyDiffuseMultiplier)(0.5, 0.75, 1.25)
        sphere.material.solidAlphaMultiplier = 0.6
        # two panes, one behind the other, both translucent: the mirror ray that passes both has two contributing hits and the sky behind them
        p = _add_quad(d, "pane", (-6.0, 2.0, -2.0), 2.0, 2.0, "camera"); p.material.solidAlphaMultiplier = 0.4
        b = _add_quad(d, "back", (-6.0, 2.0, -4.0), 3.0, 2.0, "camera"); _colour(b, (0, 153, 51)); b.material.solidAlphaMultiplier = 0.8
    elif name == "glass":
        d.lights = [far, near, below, dim]; case["view"] = dict(di_samples=2, max_lights=3)
        floor.material.reflectionFactor = 0.0
        floor.material.fogEnabled = 1; floor.material.fogMul = 2000.0; floor.material.fogOffset = -1800.0
        sphere.material.refractionFactor = 0.9; sphere.material.solidAlphaMultiplier = 0.6
        q = _add_quad(d, "slab", (-2.0, 1.0, 4.5), 1.5, 1.5, "up")                   # seen at grazing incidence: refract() returns 0 at a factor of 1.5
        q.material.refractionFactor = 1.5; q.material.solidAlphaMultiplier = 0.6
        case["passes"] = 0; case["glass"] = True
    else:
        raise KeyError(name)

    def data_at(frame):
        if by_frame is None:
            return d
        c = copy.copy(d); c.instances = by_frame[frame]
        return c
    case["data_at"] = data_at; case["name"] = name
    return case


# ---- what the rule reads of a scene ------------------------------------------------------------------------------------------------------------

_MATERIAL = ("ignoreNormalFactor", "specularExponent", "shadowRayBias", "solidAlphaMultiplier", "reflectionFactor", "reflectionFresnelFactor", "reflectionShineFactor",
             "refractionFactor", "fogMul", "fogOffset", "depthBias")


def rule_scene(data, view, frame_count, sky_described=False):
    """sky_described: `sky` is a description for tests/sky_rule.py (the cases of tests/sky_cases.py), not the one constant term."""
    from sm64rt_legacy_renderer_amd import rt64
    r = LC.rule_inputs(data)
    v3 = lambda x: (float(x.x), float(x.y), float(x.z))
    insts = []
    for inst in data.instances:
        mesh = data.meshes[inst.mesh]
        if not (mesh.flags & rt64.MESH_RAYTRACE_ENABLED):
            continue
        assert inst.normal is None and inst.specular is None                  # normal and specular maps: out of scope
        m = inst.material
        mat = {k: float(getattr(m, k)) for k in _MATERIAL}
        mat.update(lightGroupMaskBits=int(m.lightGroupMaskBits), fogEnabled=int(m.fogEnabled), selfLight=v3(m.selfLight), specularColor=v3(m.specularColor),
                   fogColor=v3(m.fogColor), diffuseColorMix=(float(m.diffuseColorMix.x), float(m.diffuseColorMix.y), float(m.diffuseColorMix.z), float(m.diffuseColorMix.w)))
        idx = np.asarray(mesh.indices, dtype=np.int64)
        tex = None
        if mat["diffuseColorMix"][3] != 1.0:
            t = data.textures[inst.diffuse]
            assert t.format == rt64.TEXTURE_FORMAT_RGBA8                          # one level as created (no generate_mipmaps)
            tex = dict(levels=[np.asarray(t.data)], uv=mesh.vertices["uv"].astype(np.float64)[idx].reshape(-1, 3, 2), filter=int(data.shader_filter),
                       ha=int(data.shader_haddr), va=int(data.shader_vaddr))
        insts.append(dict(texture=tex, material=mat, triangles=r["triangles"][len(insts)], normals=mesh.vertices["normal"].astype(np.float64)[idx].reshape(-1, 3, 3),
                          transform=np.asarray(inst.transform, dtype=np.float32), cull=not (inst.flags & rt64.INSTANCE_DISABLE_BACKFACE_CULLING)))
    cam = r["camera"]
    fov, zn, zf = cam["fov"], cam["near"], cam["far"]
    sy = 1.0 / np.tan(0.5 * fov); sx = sy / (W / H); rng = zf / (zn - zf)
    proj = np.zeros((4, 4)); proj[0, 0] = sx; proj[1, 1] = sy; proj[2, 2] = rng; proj[2, 3] = -1.0; proj[3, 2] = rng * zn
    sky = [light_rule.F(0.0)] * 3
    if data.sky is not None and sky_described:
        e = data.desc
        assert data.textures[data.sky].format == rt64.TEXTURE_FORMAT_RGBA8
        sky = dict(texels=np.asarray(data.textures[data.sky].data), multiplier=v3(e.skyDiffuseMultiplier), hsl=v3(e.skyHSLModifier), yawOffset=float(e.skyYawOffset),
                   camera=dict(view=np.asarray(data.view, dtype=np.float32), width=W, height=H, jitter=(0.0, 0.0)), tiled=False, mutate=None)
    elif data.sky is not None:
        t = data.textures[data.sky].data
        assert (t == t[0, 0]).all() and t[0, 0, 3] == 255                     # one texel value, opaque: sky_finish(texel) whatever the UV
        e = data.desc
        assert (e.skyHSLModifier.x, e.skyHSLModifier.y, e.skyHSLModifier.z) == (0.0, 0.0, 0.0)
        sky = [light_rule.mul(light_rule.F(t[0, 0, c] / 255.0, 2.0 * light_rule.U * t[0, 0, c] / 255.0), float(x)) for c, x in enumerate(v3(e.skyDiffuseMultiplier))]
    return dict(instances=insts, lights=r["lights"], ambientBase=v3(data.desc.ambientBaseColor), ambientNoGI=v3(data.desc.ambientNoGIColor), sky=sky,
                bluenoise=data.bluenoise, frameCount=int(frame_count), diSamples=int(view["di_samples"]), viewProj=cam["view"] @ proj, eyeDiffuse=r["eye_diffuse"],
                shadow=light_rule.BruteForceShadows(r["triangles"]))


# ---- sessions ----------------------------------------------------------------------------------------------------------------------------------

def oracle_sessions(case):
    """{(k, frame): images} of the CPU oracle for k = 0 .. passes, and {(k, frame): rays}."""
    from oracle import oracle_py
    out, rays = {}, {}
    for k in range(case["passes"] + 1):
        first = case["data_at"](0)
        o = oracle_py.OracleScene(first)
        try:
            now = list(first.instances)
            for f in range(case["frames"]):
                d = case["data_at"](f)
                for j, inst in enumerate(d.instances):
                    if inst is not now[j]:
                        o.set_instance(j, inst); now[j] = inst
                ref = o.render(W, H, images=f in case["compared"], diSamples=case["view"]["di_samples"], maxLights=case["view"]["max_lights"], maxReflections=k)
                if f in case["compared"]:
                    assert ref["pixelJitter"] == (0.0, 0.0)
                    out[(k, f)] = {key: ref[name] for key, name in ORACLE_IMAGES.items()}
                    rays[(k, f)] = (ref["counters"]["reflectionRays"], ref["counters"]["refractionRays"])
        finally:
            o.close()
    return out, rays


def gpu_sessions(rt64_lib, case, options=None, view=None):
    """The same sessions on the device, with device options (a kernel path) and view-description overrides."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    out, rays = {}, {}
    for k in range(case["passes"] + 1):
        first = case["data_at"](0)
        s = sample_scene.Rt64Scene(rt64_lib, first, W, H, hip_device=0)
        try:
            s.set_view_description(**dict(case["view"], **(view or {})))
            assert s.option("max_reflections", k) and s.option("count_traversal", 1)          # (the frame's ray counters are kept only with count_traversal)
            for key, v in (options or {}).items():
                assert s.option(key, v), key
            now = list(first.instances)
            for f in range(case["frames"]):
                d = case["data_at"](f)
                for j, inst in enumerate(d.instances):
                    if inst is not now[j]:
                        s.set_instance(j, inst); now[j] = inst
                s.data = d
                s.draw()
                if f in case["compared"]:
                    st = s.stats()
                    rays[(k, f)] = (int(st.reflectionRays), int(st.refractionRays))
                    out[(k, f)] = {key: s.readback(getattr(rt64, "IMAGE_" + name)) for key, name in GPU_IMAGES.items()}
        finally:
            s.close()
    return out, rays


# ---- holding a side to the rule ----------------------------------------------------------------------------------------------------------------

def _state_ratio(stored, pair):
    v, b = pair
    dev = np.abs(np.asarray(stored, dtype=np.float64)[..., :3] - v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dev == 0.0, 0.0, dev / b)
    return np.where(np.isnan(r), np.inf, r).max(axis=-1)


def run_pass(case, sess, frame, k, mutate=None):
    """The rule for reflection pass k of a compared frame on session k's stored images."""
    a = sess[(k, frame)]
    scene = rule_scene(case["data_at"](frame), case["view"], frame)
    return M.reflection_pass(scene, a["position"], a["view"], a["normal"], a["id"], a["reflection"], mutate=mutate)


def run_glass(case, sess, frame, mutate=None):
    a = sess[(0, frame)]
    scene = rule_scene(case["data_at"](frame), case["view"], frame)
    pristine = a["refraction"].copy(); pristine[..., :3] = 0.0            # (0, 0, 0, alpha) as PrimaryRayGen leaves it
    return M.refraction_pass(scene, a["position"], a["view"], a["normal"], a["id"], pristine, mutate=mutate)


def judge_pass(rule, a, b):
    """One reflection pass against the next session's stored images b (a: this session's).  A pixel is `bad` when, the rule having decided it, its REFLECTION value is at
    or outside the bound, it goes on to the next pass where the rule says it stops (or the reverse), its continuation state (id exactly; position, direction, normal within
    bound) is not the rule's, or -- taken by no pass, or its ray ending on no surface -- its state bytes changed.  Returns dict(ratio, mean, bad, undecided, takes, on, state)."""
    takes, decided = rule["takes"], rule["decided"]
    ok = takes & decided
    dev = np.abs(np.asarray(b["reflection"], dtype=np.float64) - rule["value"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(dev == 0.0, 0.0, dev / rule["bound"])
    ratio = np.where(np.isnan(ratio), np.inf, ratio).max(axis=-1)
    bad = (ok & (ratio >= 1.0)) | (~takes & (ratio > 0.0))
    hit = ok & rule["has_hit"]
    bad |= ok & (rule["goes_on"] != ((b["id"] >= 0) & (b["reflection"][..., 3] > M.EPSILON)))
    bad |= hit & (b["id"] != rule["state_id"])
    ratios = {}
    for key, name in (("position", "state_position"), ("view", "state_direction"), ("normal", "state_normal")):
        r = _state_ratio(b[key], rule[name])
        bad |= hit & (r >= 1.0)
        ratios[key] = float(r[hit].max()) if hit.any() else 0.0
    keep = ~takes | (ok & ~rule["has_hit"])
    for key in STATE:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        same = (x == y) if x.ndim == 2 else (x.view(np.uint32) == y.view(np.uint32)).all(axis=-1)
        bad |= keep & ~same
    return dict(ratio=float(ratio[ok].max()) if ok.any() else 0.0, mean=float(ratio[ok].mean()) if ok.any() else 0.0, bad=int(bad.sum()),
                undecided=int((takes & ~decided).sum()), takes=int(takes.sum()), state=ratios, on=int((rule["goes_on"] & ok).sum()))


def judge_glass(rule, stored):
    takes, decided = rule["takes"], rule["decided"]
    worst, outside, mean = M.compare(stored, rule["value"], rule["bound"], decided, takes)
    return dict(ratio=worst, mean=mean, bad=outside, undecided=int((takes & ~decided).sum()), takes=int(takes.sum()))


def hold(case, sess, rays, side, rules=None, images_only=False, log=print):
    """Every compared frame and pass of a case's sessions against the rule; asserts the conditions of the tests, returns the report rows.  rules: a cache
    {(frame, k or "glass"): rule result} filled here (the rule runs once per case on the default path; a kernel path whose inputs are the same bytes reuses it)."""
    rules = {} if rules is None else rules
    rows = []
    name = case["name"]
    need = SHARES[name]
    for f in case["compared"]:
        base = sess[(0, f)]
        for k in range(1, case["passes"] + 1):                                  # the images no pass writes
            for key in () if images_only else UNTOUCHED:
                assert np.array_equal(sess[(k, f)][key], base[key]), (key, k, f)
        expected_rays, slack = 0, 0
        for k in range(case["passes"]):
            a, b = sess[(k, f)], sess[(k + 1, f)]
            if (f, k) not in rules:
                rules[(f, k)] = run_pass(case, sess, f, k)
            rule = rules[(f, k)]
            j = judge_pass(rule, a, b)
            cap = int(UNDECIDED_CAP * j["takes"])
            rows.append("mirror_rule %-6s %-16s frame %d pass %d  ratio=%.6f mean=%.6f state pos=%.3f dir=%.3f nrm=%.3f  takes=%d on=%d undecided=%d %s"
                        % (side, name, f, k, j["ratio"], j["mean"], j["state"]["position"], j["state"]["view"], j["state"]["normal"], j["takes"], j["on"], j["undecided"],
                           {x: y for x, y in rule["info"]["undecided"].items() if y}))
            log(rows[-1])
            assert j["bad"] == 0 and j["ratio"] < 1.0 and max(j["state"].values()) < 1.0, (name, f, k, j)
            assert j["undecided"] <= cap, (name, f, k, j["undecided"], cap)
            expected_rays += j["takes"]
            if k == 0 and "mirrored" in need:
                t = rule["takes"]
                assert j["takes"] >= need["mirrored"] and rule["info"]["lit_surface"][t].mean() >= need["surface"], (j["takes"], rule["info"]["lit_surface"][t].mean())
                assert j["on"] >= need.get("on", 0.0) * j["takes"], (j["on"], j["takes"])
                three, tex = float((rule["info"]["contributing"][t] >= 3).mean()), float(rule["info"]["textured"][t].mean())
                if "three" in need or "textured" in need:
                    log("mirror_rule %-6s %-16s shares: three or more contributing hits %.3f, a texel in the colour %.3f" % (side, name, three, tex))
                assert three >= need.get("three", 0.0) and tex >= need.get("textured", 0.0), (three, tex)
            # the rays the side counted in the session that runs passes 0 .. k: every pixel each pass takes.  EQUAL, with no allowance for undecided pixels: which pixels a
            # pass takes is read from the stored inputs, not predicted (the prediction, goes_on, is held per pixel in judge_pass)
            assert rays[(k + 1, f)][0] == expected_rays, (name, f, k, rays[(k + 1, f)], expected_rays)
        if case["glass"]:
            if (f, "glass") not in rules:
                rules[(f, "glass")] = run_glass(case, sess, f)
            rule = rules[(f, "glass")]
            j = judge_glass(rule, base["refraction"])
            worst, outside, mean, und, n, takes = j["ratio"], j["bad"], j["mean"], j["undecided"], j["takes"], rule["takes"]
            tir = float(rule["total_internal"][takes].mean()) if n else 0.0
            rows.append("mirror_rule %-6s %-16s frame %d glass   ratio=%.6f mean=%.6f takes=%d total_internal=%.3f undecided=%d %s"
                        % (side, name, f, worst, mean, n, tir, und, {x: y for x, y in rule["info"]["undecided"].items() if y}))
            log(rows[-1])
            assert outside == 0 and worst < 1.0, (name, f, worst, outside)
            assert und <= int(UNDECIDED_CAP * n), (name, und, n)
            assert n >= need["glass"] and tir >= need["total_internal"], (n, tir)
            assert rays[(0, f)][1] == n, (rays[(0, f)], n)
    return rows
