"""Scenes and rays of the radiance queries (rules W1-W12) for tests/test_gpu_radiance_query.py.  TEST INFRASTRUCTURE.

Every case is a sheet stack of tests/layers_cases.py -- K translucent sheets of alpha 0.2, 0.4, 0.6 above the camera, over the sample scene's floor, under its
sky and its one light -- with what the resolve of a secondary ray reads beyond a layer's weight switched on sheet by sheet:
  stack_3, stack_8   the stacks with flat colours: every layer lit, no fog
  fog_8              sheets 1, 4, 7 lie in fog (three colours, fogMul 12 / 20 / 30, fogOffset 0 / 1 / -0.5): a fogged translucent layer in front of lit ones
  unlit_8            sheets 0, 3, 6, 7 have lightGroupMaskBits 0 and a selfLight of their own: from below sheet 0 is the first layer and sheet 7 the last contributor
  edge_8             layout "ignored_hits": a texture-edge cutout second from the top, sheets that turn their backs
  lights_8           a second light under the floor, which blocks it for every sheet, and a third that no sheet's mask admits
  caster_8           every sheet's shadow alpha is a quarter of its alpha: translucent shadow casters, a visibility that falls sheet by sheet
  nosky_3            the scene without a sky texture and without a raster background: nothing behind the layers
  sky_3              a described sky (tests/sky_cases.py's kind: a generated 64 x 32 texture whose alpha runs from 0 to 1, a multiplier, an HSL modifier, a yaw
                     offset) over no raster background: the rays that miss everything leave into a translucent sky
  faint_12           sheets 0..9 and 11 of alpha 0.6, sheet 10 of alpha 1 / 255: from below its weight is 0.4^10 / 255 = 4.1e-7, under the 1e-6 gate
  mirror_3           tests/mirror_cases.py's base scene (the sample scene without background instances, normal and specular maps; flat colours), the sphere
                     translucent (0.6) and in fog through mirror_cases._with: closed surfaces, curved normals, back faces
Rays are layers_cases.rays_of's: down through the stack, up from under it, grazing its edges, from inside it, short windows, Q6-invalid; the ones that start above
the top sheet and point up, added here, miss everything into the sky.
"""
import copy

import numpy as np

import layers_cases as LC
import test_oracle_kbuffer as KB

W, H = LC.W, LC.H
FOG = {1: ((0.9, 0.2, 0.1), 12.0, 0.0), 4: ((0.1, 0.8, 0.3), 20.0, 1.0), 7: ((0.2, 0.3, 0.9), 30.0, -0.5)}
UNLIT = {0: (0.3, 0.1, 0.0), 3: (0.0, 0.2, 0.4), 6: (0.25, 0.25, 0.0), 7: (0.1, 0.0, 0.2)}
NAMES = ("stack_3", "stack_8", "fog_8", "unlit_8", "edge_8", "lights_8", "caster_8", "nosky_3", "sky_3", "mirror_3", "faint_12")
SEEDS = {name: 101 + 7 * k for k, name in enumerate(NAMES)}


def case(sample_data, name):
    """-> (SceneData, number of sheets)"""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    K = int(name.rsplit("_", 1)[1])
    if name == "mirror_3":
        import mirror_cases
        d, sphere, floor = mirror_cases._base(sample_data)
        ball = mirror_cases._with(sphere, solidAlphaMultiplier=0.6, fogEnabled=1, fogMul=25.0, fogOffset=0.5)
        ball.diffuse = floor.diffuse          # an RGBA8 texture under the flat colour
        d.instances[d.instances.index(sphere)] = ball
        floor.material.reflectionFactor = 0.0
        floor.material.fogEnabled = 1; floor.material.fogMul = 60.0; floor.material.fogOffset = 0.0          # the last contributor of most rays, in fog as well
        return d, K
    d = LC.stack_case(sample_data, K, "ignored_hits" if name == "edge_8" else "instances")
    sheets = d.instances[d.floor_instance + 1:]
    # Flat colours (diffuseColorMix.w = 1, as tests/mirror_cases.py paints its scenes), a quarter of a UNORM8 step above a step: the frame's store moves each by
    # 0.25 / 255, far from a tie.  A colour that comes through a texture carries the sampler's bound, and 255 x that bound reaches the store's rounding boundary on
    # a tenth of the rays; alpha still comes from the vertex colours and solidAlphaMultiplier.
    for k, inst in enumerate([d.instances[d.floor_instance]] + list(sheets)):
        byte = lambda j: (((53 * k + 71 * j + 40) % 200) + 30 + 0.25) / 255.0
        inst.material.diffuseColorMix = rt64.VECTOR4(byte(0), byte(1), byte(2), 1.0)
    if name == "faint_12":
        for k, inst in enumerate(sheets):
            inst.material.solidAlphaMultiplier = 1.0 / 255.0 if k == 10 else 0.6
    elif name == "fog_8":
        for k, (colour, mul, offset) in FOG.items():
            m = sheets[k].material
            m.fogEnabled = 1; m.fogColor = rt64.VECTOR3(*colour); m.fogMul = mul; m.fogOffset = offset
    elif name == "unlit_8":
        for k, self_light in UNLIT.items():
            sheets[k].material.lightGroupMaskBits = 0; sheets[k].material.selfLight = rt64.VECTOR3(*self_light)
    elif name == "lights_8":
        first = d.lights[-1]
        under, other = copy.copy(first), copy.copy(first)
        under.position = rt64.VECTOR3(1.0, -6.0, -2.0); under.diffuseColor = rt64.VECTOR3(0.2, 0.9, 0.4); under.attenuationRadius = 60.0
        other.groupBits = 0x80000000; other.diffuseColor = rt64.VECTOR3(5.0, 5.0, 5.0)
        for inst in d.instances:          # the sample's materials admit every group: the sheets and the floor keep to the default one
            inst.material.lightGroupMaskBits = rt64.LIGHT_GROUP_DEFAULT
        d.lights = list(d.lights) + [under, other]
    elif name == "caster_8":
        for inst in sheets:
            inst.material.shadowAlphaMultiplier = 0.25
    elif name in ("nosky_3", "sky_3"):
        for inst in d.instances:          # no raster background: what lies behind the layers is the sky alone
            inst.flags &= ~rt64.INSTANCE_RASTER_BACKGROUND
        d.sky = None
        if name == "sky_3":
            import ctypes
            y, x = np.mgrid[0:32, 0:64]
            texels = np.stack([(x * 4) % 256, (y * 8) % 256, (x * 3 + y * 5) % 256, (x * 4 + y) % 256], axis=-1).astype(np.uint8)
            d.textures = list(d.textures) + [sample_scene.TextureData("sky-alpha", rt64.TEXTURE_FORMAT_RGBA8, texels, 64, 32)]
            d.sky = len(d.textures) - 1
            desc = type(d.desc)(); ctypes.memmove(ctypes.byref(desc), ctypes.byref(d.desc), ctypes.sizeof(desc)); d.desc = desc
            d.desc.skyDiffuseMultiplier = rt64.VECTOR3(0.8, 1.1, 0.9); d.desc.skyHSLModifier = rt64.VECTOR3(0.1, -0.2, 0.15); d.desc.skyYawOffset = 0.7
    return d, K


def rays_of(K, seed, per_kind=48, name=None, data=None):
    """layers_cases.rays_of's kinds and, in front of them, per_kind rays that leave upwards from above the top sheet: they miss everything."""
    rng = np.random.default_rng(seed + 1000)
    m = per_kind
    if name == "mirror_3":          # towards the sphere (centre (0, 0.5, 0), radius 2.55) from a shell around it: through it onto the floor, past it, and a sixth upwards
        n = 6 * m
        ang, rad = rng.uniform(0.0, 2.0 * np.pi, size=n), rng.uniform(6.0, 12.0, size=n)
        o = np.stack([rad * np.cos(ang), rng.uniform(0.6, 6.0, size=n), rad * np.sin(ang)], axis=1)
        target = np.array([0.0, 0.5, 0.0]) + rng.uniform(-3.2, 3.2, size=(n, 3))
        d = (target - o) * 10.0 ** rng.uniform(-0.5, 0.5, size=(n, 1))
        d[:m, 1] = np.abs(d[:m, 1]) + 0.5 * np.linalg.norm(d[:m], axis=1)
        r = np.zeros((n, 8), dtype=np.float32); r[:, 0:3] = o; r[:, 4:7] = d; r[:, 7] = 1000.0
        return np.ascontiguousarray(np.concatenate([r, LC.rays_of(K, seed, per_kind)[-8:]]))
    top = KB.sheet_height(K - 1) + KB.SLOPE * 80.0
    up = np.zeros((m, 8), dtype=np.float32)
    up[:, 0:3] = rng.uniform((-9.0, top + 0.5, -9.0), (9.0, top + 2.0, 9.0), size=(m, 3))
    d = np.concatenate([rng.uniform(-1.5, 1.5, size=(m, 1)), rng.uniform(0.05, 1.0, size=(m, 1)), rng.uniform(-1.5, 1.5, size=(m, 1))], axis=1)
    up[:, 4:7] = d * 10.0 ** rng.uniform(-0.5, 0.5, size=(m, 1))
    up[:, 3] = 0.0; up[:, 7] = 1000.0
    return np.ascontiguousarray(np.concatenate([up, LC.rays_of(K, seed, per_kind)]))

