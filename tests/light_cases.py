"""Scene cases of the direct-light rule tests (tests/test_light_rule.py on the CPU oracle, tests/test_gpu_light_rule.py on the GPU): variants of the sample
scene at 88 x 72 -- both sides over 64, so the blue-noise address wraps; neither a multiple of the 16-pixel tile -- and what tests/light_rule.py needs to
know about each.  Every coordinate added here is a small multiple of a power of two, so the float64 world-space triangles are the float32 ones exactly."""
import copy
import ctypes as C

import numpy as np

import light_rule

W, H = 88, 72

# case -> (scene variant, view description, frames drawn: the compared frame is the last one, frameCount = frames - 1)
CASES = ("one", "four", "twenty", "pick-one", "masks", "falloff", "offsets", "material", "radius-0", "radius-1", "radius-4", "radius-2p",
         "frames-0", "frames-1", "frames-62", "frames-63", "frames-64")

# what makes a case worth running, as shares of its shaded pixels measured on the rule: at least this much in shadow (some sample of some drawn light occluded), with
# more than one light drawn, and -- falloff only -- beyond the radius of at least four of its lights (the three local ones and the one that reaches nothing)
SHARES = {
    "one": (0.01, 0.0, 0.0), "four": (0.30, 0.95, 0.0), "twenty": (0.50, 0.95, 0.0), "pick-one": (0.03, 0.0, 0.0), "masks": (0.08, 0.95, 0.0),
    "falloff": (0.05, 0.95, 0.10), "offsets": (0.25, 0.95, 0.0), "material": (0.30, 0.95, 0.0),
    "radius-0": (0.15, 0.95, 0.0), "radius-1": (0.15, 0.95, 0.0), "radius-4": (0.15, 0.95, 0.0), "radius-2p": (0.15, 0.95, 0.0),
    "frames-0": (0.08, 0.95, 0.0), "frames-1": (0.08, 0.95, 0.0), "frames-62": (0.08, 0.95, 0.0), "frames-63": (0.08, 0.95, 0.0), "frames-64": (0.08, 0.95, 0.0),
}


def shares(info):
    """(in shadow, more than one light drawn, beyond four radii) as shares of the shaded pixels of a rule result."""
    lit = info["lit"]
    return float(info["in_shadow"][lit].mean()), float((info["draws"][lit] > 1).mean()), float((info["radii_outside"][lit] >= 4).mean())


# the case built to catch each wrong variant of the rule (tests/test_light_rule.py tries it first)
MUTATION_CASE = {
    "select_slot_plus_one": "pick-one", "sample_slot_up": "radius-4", "invprob_always": "four", "not_zeroed": "four", "radius_at_zero": "radius-0",
    "offset_added": "offsets", "tmin_no_bias": "offsets", "ndotl_unclamped": "four", "raydir_normalised": "material", "eye_spec_unsaturated": "material",
    "cap_scanned": "twenty", "bn_no_xmod": "radius-4",
}


def _light(stock, pos, col, radius=40.0, exponent=2.0, point_radius=0.0, shadow_offset=0.0, bits=1, spec=None):
    from sm64rt_legacy_renderer_amd import rt64
    l = rt64.LIGHT(); C.memmove(C.byref(l), C.byref(stock), C.sizeof(rt64.LIGHT))
    l.position = rt64.VECTOR3(*pos); l.diffuseColor = rt64.VECTOR3(*col); l.specularColor = rt64.VECTOR3(*(spec or col))
    l.attenuationRadius = radius; l.attenuationExponent = exponent; l.pointRadius = point_radius; l.shadowOffset = shadow_offset; l.groupBits = bits
    return l


def _add_quad(d, centre, half=0.75):
    """A thin horizontal occluder: two triangles facing up, their own mesh and instance (the floor's textures and the base material)."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    floor = next(i for i in d.instances if i.name == "floor")
    v = d.meshes[floor.mesh].vertices[:4].copy()
    v["position"] = [(-half, 0.0, -half, 1.0), (half, 0.0, -half, 1.0), (-half, 0.0, half, 1.0), (half, 0.0, half, 1.0)]
    d.meshes.append(sample_scene.MeshData("quad%d" % len(d.meshes), rt64.MESH_RAYTRACE_ENABLED, v, np.array([2, 1, 0, 1, 2, 3], dtype=np.uint32)))
    t = np.eye(4, dtype=np.float32); t[3, :3] = centre
    q = copy.copy(floor); q.name = "quad%d" % len(d.instances); q.mesh = len(d.meshes) - 1; q.transform = t; q.previous_transform = t
    q.material = sample_scene.base_material()
    d.instances.append(q)
    return q


def make_case(sample_data, name):
    """(SceneData, view description, frames) of a case."""
    from sm64rt_legacy_renderer_amd import sample_scene
    d = copy.copy(sample_data)
    d.desc = type(sample_data.desc)(); C.memmove(C.byref(d.desc), C.byref(sample_data.desc), C.sizeof(d.desc))
    d.instances = [copy.copy(i) for i in sample_data.instances]
    for i in d.instances:
        i.material = sample_scene.copy_material(i.material)
    d.meshes = list(sample_data.meshes)
    stock = sample_data.lights[0]
    sphere = next(i for i in d.instances if i.name == "sphere"); floor = next(i for i in d.instances if i.name == "floor")
    far = _light(stock, (15000.0, 30000.0, 15000.0), (0.8, 0.75, 0.65), radius=1e9, exponent=1.0, point_radius=5000.0)
    near = [_light(stock, (-6.0, 4.0, 3.0), (0.9, 0.2, 0.1), point_radius=0.5), _light(stock, (5.0, 3.0, 6.0), (0.1, 0.3, 0.9), point_radius=0.5),
            _light(stock, (0.0, 8.0, -4.0), (0.2, 0.7, 0.2), point_radius=0.5)]
    below = _light(stock, (0.5, -3.0, -4.0), (0.3, 0.6, 0.3), point_radius=0.25)      # under the floor: N.L < 0 on the floor, nothing between them
    # The last candidate of a pixel is dim wherever more than one draw is made.  Once the last slot has been drawn and zeroed, a later draw whose blue-noise byte is
    # 255 compares r = remaining with a running sum that is mathematically equal to it: float32 decides that by the order of its additions and no float64 rule can.
    # A dim last candidate is drawn first almost only by such a byte, which keeps those pixels rare.
    dim = _light(stock, (0.0, 6.0, 8.0), (0.0002, 0.0002, 0.0002))
    view, frames = dict(di_samples=0, max_lights=12), 1
    if name == "one":
        pass                                                                  # the stock light: one candidate
    elif name == "four":
        d.lights = [far, near[0], below, dim]; view = dict(di_samples=2, max_lights=3)
    elif name == "twenty":
        # light 0 fails the mask, light 1 has no colour; 2 .. 19 are admissible: 18, so the cap of 16 ADMITTED stops at light 17, a cap of 16 scanned at light 15
        # ignoreNormalFactor 1 admits every light that passes the mask at every pixel (the surface bias is 1.707 whatever the normal), so the cap is hit everywhere.
        # frameCount 9: among the slices 9 .. 20 few tile positions hold the byte 255 twice (see the note on the dim last candidate above).
        for i in d.instances:
            i.material.lightGroupMaskBits = 5; i.material.ignoreNormalFactor = 1.0
        ls = [_light(stock, (2.0, 5.0, 4.0), (0.9, 0.9, 0.9), bits=2), _light(stock, (-2.0, 5.0, 4.0), (0.0, 0.0, 0.0), bits=1)]
        for k in range(18):
            a = 2.0 * np.pi * k / 18.0
            ls.append(_light(stock, (float(np.float32(7.0 * np.cos(a))), 2.0 + 0.25 * (k % 5), float(np.float32(1.0 + 6.0 * np.sin(a)))),
                             (0.05 + 0.03 * (k % 3), 0.06 + 0.02 * (k % 4), 0.05 + 0.04 * (k % 2)), radius=30.0, exponent=1.0 + 0.5 * (k % 3),
                             point_radius=0.25, bits=1 if k % 2 else 4))
        for k in (17, 18, 19):                                                # whichever is admitted last is dim (see above); 18 and 19 lie beyond the cap where 2 .. 17 are all admitted
            ls[k] = _light(stock, (float(k - 18), 6.0, 8.0), (0.0002, 0.0002, 0.0002), radius=30.0, bits=1)
        d.lights = ls; view = dict(di_samples=1, max_lights=12); frames = 10
    elif name == "pick-one":
        d.lights = [far] + near; view = dict(di_samples=0, max_lights=1)
    elif name == "masks":
        sphere.material.lightGroupMaskBits = 0; floor.material.lightGroupMaskBits = 2
        _add_quad(d, (-2.0, 1.0, 2.0)).material.lightGroupMaskBits = 5
        d.lights = [_light(stock, (-6.0, 4.0, 3.0), (0.9, 0.2, 0.1), bits=1), _light(stock, (5.0, 3.0, 6.0), (0.1, 0.3, 0.9), bits=2),
                    _light(stock, (0.0, 8.0, -4.0), (0.2, 0.7, 0.2), bits=4), _light(stock, (-3.0, 6.0, 5.0), (0.5, 0.5, 0.2), bits=2),
                    _light(stock, (0.0, 6.0, 8.0), (0.0002, 0.0002, 0.0002), bits=7)]
    elif name == "falloff":
        # exponent 0: pow(0, 0) = 1, so that light reaches every pixel whatever its radius says; the last one's radius excludes every pixel
        d.lights = [_light(stock, (-2.0, 3.0, 2.0), (0.9, 0.3, 0.2), radius=6.0, exponent=2.0), _light(stock, (3.0, 2.0, 3.0), (0.2, 0.4, 0.9), radius=5.0, exponent=0.5),
                    _light(stock, (0.0, 4.0, -6.0), (0.3, 0.8, 0.3), radius=7.0, exponent=8.0), far,
                    _light(stock, (2.0, 1.0, 6.0), (0.0002, 0.0002, 0.0001), radius=4.0, exponent=0.0), _light(stock, (0.0, 50.0, 0.0), (1.0, 1.0, 1.0), radius=10.0, exponent=1.0)]
        view = dict(di_samples=0, max_lights=2)
    elif name == "offsets":
        floor.material.shadowRayBias = 1.9                                    # tmin = 2.0 for rays that start on the floor
        _add_quad(d, (3.0, 3.5, 2.0))                                         # 0.5 under light 0, inside its shadowOffset: must not shadow what lies under it
        _add_quad(d, (-2.0, 1.0, 2.0))                                        # 1.0 over the floor: nearer than tmin along steep rays (no shadow), farther along flat ones (shadow)
        d.lights = [_light(stock, (3.0, 4.0, 2.0), (0.8, 0.7, 0.5), radius=30.0, shadow_offset=1.0), _light(stock, (2.0, 6.0, 3.0), (0.3, 0.5, 0.8), radius=30.0),
                    _light(stock, (-9.0, 2.0, 2.0), (0.4, 0.4, 0.4), radius=30.0, shadow_offset=0.25), dim]
        view = dict(di_samples=0, max_lights=4)
    elif name == "material":
        sphere.material.ignoreNormalFactor = 0.5; sphere.material.specularExponent = 64.0; sphere.material.selfLight = type(sphere.material.selfLight)(0.05, 0.02, 0.0)
        floor.material.ignoreNormalFactor = 1.0; floor.material.specularExponent = 5.0
        _add_quad(d, (-2.0, 1.0, 2.0))                                        # specularExponent 1
        d.desc.eyeLightDiffuseColor = type(d.desc.eyeLightDiffuseColor)(0.3, 0.2, 0.1); d.desc.eyeLightSpecularColor = type(d.desc.eyeLightSpecularColor)(0.5, 0.6, 0.7)
        d.lights = near + [dim]
    elif name.startswith("radius-"):
        ds = {"radius-0": 0, "radius-1": 1, "radius-4": 4, "radius-2p": 2}[name]
        d.lights = [far] + near[:2] + [dim]
        if name == "radius-2p":
            d.lights = [_light(stock, (l.position.x, l.position.y, l.position.z), (l.diffuseColor.x, l.diffuseColor.y, l.diffuseColor.z), radius=l.attenuationRadius,
                               exponent=l.attenuationExponent, point_radius=0.0) for l in d.lights]
        view = dict(di_samples=ds, max_lights=12)
    elif name.startswith("frames-"):
        d.lights = [far] + near + [dim]; view = dict(di_samples=2, max_lights=2); frames = int(name.split("-")[1]) + 1
    else:
        raise KeyError(name)
    return d, view, frames


def rule_inputs(data):
    """What the rule reads of a scene: materials and world-space triangles of the ray-traced instances (in instance-id order), lights, eye light, camera."""
    from sm64rt_legacy_renderer_amd import rt64
    mats, tris = [], []
    for inst in data.instances:
        mesh = data.meshes[inst.mesh]
        if not (mesh.flags & rt64.MESH_RAYTRACE_ENABLED):
            continue
        m = inst.material
        mats.append(dict(lightGroupMaskBits=int(m.lightGroupMaskBits), ignoreNormalFactor=float(m.ignoreNormalFactor), specularExponent=float(m.specularExponent),
                         shadowRayBias=float(m.shadowRayBias), selfLight=(float(m.selfLight.x), float(m.selfLight.y), float(m.selfLight.z))))
        p = mesh.vertices["position"].astype(np.float64); p[:, 3] = 1.0
        world = (p @ np.asarray(inst.transform, dtype=np.float64))[:, :3]
        tris.append(world[np.asarray(mesh.indices, dtype=np.int64)].reshape(-1, 3, 3))
    lights = [dict(position=(l.position.x, l.position.y, l.position.z), diffuseColor=(l.diffuseColor.x, l.diffuseColor.y, l.diffuseColor.z),
                   attenuationRadius=l.attenuationRadius, pointRadius=l.pointRadius, specularColor=(l.specularColor.x, l.specularColor.y, l.specularColor.z),
                   shadowOffset=l.shadowOffset, attenuationExponent=l.attenuationExponent, groupBits=int(l.groupBits)) for l in data.lights]
    e = data.desc
    return dict(materials=mats, triangles=tris, lights=lights,
                eye_diffuse=(e.eyeLightDiffuseColor.x, e.eyeLightDiffuseColor.y, e.eyeLightDiffuseColor.z),
                eye_specular=(e.eyeLightSpecularColor.x, e.eyeLightSpecularColor.y, e.eyeLightSpecularColor.z),
                camera=dict(view=np.asarray(data.view, dtype=np.float64), fov=float(np.float32(data.fov)), near=float(np.float32(data.near)), far=float(np.float32(data.far)),
                            width=W, height=H, jitter=(0.0, 0.0)))


def run_rule(data, view, frame_count, position, normal, specular, instance_id, mutate=None):
    """The rule on one frame's stored G-buffer.  Returns (value, bound, decided, info)."""
    r = rule_inputs(data)
    shadow = light_rule.BruteForceShadows(r["triangles"])
    return light_rule.direct_light(position, normal, specular, instance_id, r["materials"], r["lights"], r["eye_diffuse"], r["eye_specular"],
                                   view["max_lights"], view["di_samples"], frame_count, data.bluenoise, r["camera"], shadow, mutate=mutate)


def compare(stored, value, bound, decided):
    """(largest deviation / bound over the decided pixels, pixels outside the bound, undecided share of the shaded pixels, mean deviation / bound) of a stored
    DIRECT_LIGHT_RAW image."""
    lit = value[..., 3] > 0.5
    dev = np.abs(stored.astype(np.float64)[..., :3] - value[..., :3])
    ok = decided & lit
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound[..., :3] > 0, dev / bound[..., :3], np.where(dev > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio).max(axis=-1)
    worst = float(ratio[ok].max()) if ok.any() else 0.0
    return worst, int((ratio[ok] >= 1.0).sum()), float((~decided & lit).sum()) / max(int(lit.sum()), 1), float(ratio[ok].mean()) if ok.any() else 0.0
