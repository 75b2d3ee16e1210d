"""The scenes the direct-light records are checked on (tests/test_lighting_rule.py on the CPU, tests/test_gpu_lighting_query.py on the GPU).  TEST INFRASTRUCTURE.

Each case is (scene data, ray seed, device options, layer heights or None).  Six are light_cases.make_case's -- its lights and materials already reach the cap of
16, the mask of 0, exponent 0, shadowOffset and the eye light -- built on material_cases.small_sample, whose textures are small RGBA8 images the material rule can
read.  Four are added: light_cases' near lights over alpha_cases' translucent veils and over its texture-edge fence, the sample's normal and specular maps under
generated mip chains with one lod per ray, and 20 admissible lights on material_cases' 66 instances.  The rays are alpha_cases.rays_of: 2000 of
ray_rule.random_rays plus, where layers are stacked, 500 steep ones.
"""
import numpy as np

import alpha_cases as AC
import light_cases as LC
import material_cases as MC

W, H = 64, 36
FROM_LIGHT_CASES = ("one", "twenty", "masks", "falloff", "offsets", "material")
NAMES = FROM_LIGHT_CASES + ("veils", "fence", "mipped maps", "66 instances, 20 lights")
SEEDS = {"one": 401, "twenty": 402, "masks": 403, "falloff": 404, "offsets": 405, "material": 406, "veils": 407, "fence": 408, "mipped maps": 409,
         "66 instances, 20 lights": 410}

# What makes a case worth running, as shares of its real hits measured on the rule: at least this much (in shadow: some admitted light blocked or dimmed; two or
# more lights admitted; some light seen through a layer at a visibility strictly between 0 and 1; UNLIT; TRUNCATED).  Chosen like light_cases.SHARES: well under
# what the geometry gives (a third of the floor lies in some shadow; every hit of "twenty" is capped), so that a reseeded batch still passes, and above what a
# broken case -- lights that reach nothing, a mask that is never 0 -- would show.
SHARES = {
    "one": (0.01, 0.0, 0.0, 0.0, 0.0), "twenty": (0.30, 0.95, 0.0, 0.0, 0.95), "masks": (0.02, 0.30, 0.0, 0.10, 0.0), "falloff": (0.02, 0.50, 0.0, 0.0, 0.0),
    "offsets": (0.10, 0.90, 0.0, 0.0, 0.0), "material": (0.10, 0.90, 0.0, 0.0, 0.0), "veils": (0.30, 0.90, 0.20, 0.0, 0.0), "fence": (0.20, 0.90, 0.0, 0.0, 0.0),
    "mipped maps": (0.10, 0.90, 0.0, 0.0, 0.0), "66 instances, 20 lights": (0.30, 0.95, 0.0, 0.0, 0.95),
}
UNDECIDED_CAP = 0.02          # of a case's real hits: the alpha rule's cap

# the case built to catch each wrong variant of the rule
MUTATION_CASE = {
    "raydir_normalised": "material", "point_radius_used": "one", "offset_added": "offsets", "tmin_no_bias": "offsets", "ndotl_unclamped": "material",
    "cap_scanned": "twenty", "mask_zero_lit": "masks", "geometric_normal": "mipped maps", "specular_map_ignored": "mipped maps", "no_self_light": "material",
    "cutouts_block": "fence", "shadow_by_solid_multiplier": "veils",
}


def _near_lights(sample_data, count):
    stock = sample_data.lights[0]
    lights = [LC._light(stock, (-6.0, 4.0, 3.0), (0.9, 0.2, 0.1)), LC._light(stock, (5.0, 3.0, 6.0), (0.1, 0.3, 0.9)), LC._light(stock, (0.0, 8.0, -4.0), (0.2, 0.7, 0.2)),
              LC._light(stock, (1.0, 7.0, 2.0), (0.5, 0.5, 0.4), shadow_offset=0.5)]
    return lights[:count]


def make_case(sample_data, name):
    """-> (SceneData, seed, device options, layer heights or None)."""
    if name in FROM_LIGHT_CASES:
        d, _view, _frames = LC.make_case(MC.small_sample(sample_data), name)
        return d, SEEDS[name], {}, None
    if name == "veils":
        d = AC.veils(sample_data); d.lights = _near_lights(sample_data, 4)
        return d, SEEDS[name], {}, AC.VEIL_HEIGHTS
    if name == "fence":
        d = AC.fence(sample_data); d.lights = _near_lights(sample_data, 3)
        return d, SEEDS[name], {}, AC.FENCE_HEIGHTS
    if name == "mipped maps":
        d = MC.detail_scales(sample_data); d.lights = _near_lights(sample_data, 3)
        d.instances[1].material.specularExponent = 8.0; d.instances[3].material.specularExponent = 3.0
        return d, SEEDS[name], {"generate_mipmaps": 1}, None
    if name == "66 instances, 20 lights":
        d = MC.many_instances(sample_data)
        stock = sample_data.lights[0]
        for i in d.instances:
            i.material.ignoreNormalFactor = 1.0          # the surface bias is 1.707 whatever the normal: every light is admitted at every hit, the cap is hit everywhere
        # (the lights hang high above the grid: a shadow ray then crosses small spheres near its origin only, where the L7 margins are small)
        d.lights = [LC._light(stock, (float(np.float32(3.0 * np.cos(2.0 * np.pi * k / 20.0))), 8.0 + 0.25 * (k % 5), float(np.float32(3.0 * np.sin(2.0 * np.pi * k / 20.0)))),
                              (0.05 + 0.03 * (k % 3), 0.06 + 0.02 * (k % 4), 0.05 + 0.04 * (k % 2)), radius=30.0, exponent=1.0 + 0.5 * (k % 3)) for k in range(20)]
        d.lights[15] = LC._light(stock, (0.0, 9.0, 0.0), (0.0002, 0.0002, 0.0002), radius=30.0)          # the 16th candidate, the last slot of a frame's walk, is dim (light_cases says why)
        return d, SEEDS[name], {"lds_cache": 1}, None
    raise KeyError(name)


def rays_and_lods(data, seed, options, heights):
    rays = AC.rays_of(data, seed, heights)
    lods = MC.lods(seed, len(rays), True) if MC.mipmapped(options) else None
    return rays, lods


# P8's frames: after how many frames the compared one is drawn.  A pixel whose blue-noise byte is 255 at a late draw is one light_rule cannot decide (L9a); which
# pixels those are depends on the slices frameCount .. frameCount + 15 alone, so the frame number is chosen per case to keep them under L9's cap.
PICTURE_FRAMES = {"twenty": 10, "falloff": 18, "veils": 13, "fence": 6, "66 instances, 20 lights": 8}


def picture_case(sample_data, name):
    """-> (SceneData, width, height, frames) of the frame a case is held against the picture on: light_cases' scenes at its 88 x 72, the others at 64 x 36; the
    two cases that look at their layers from above are looked at from the sample's own camera instead, which sees the sphere and the floor under them, at
    88 x 72 as well (the veils leave few pixels with an opaque surface)."""
    d = make_case(sample_data, name)[0]
    if name in ("veils", "fence"):
        d.view = np.array(sample_data.view, dtype=np.float32)
    for i in d.instances:          # the oracle's binding draws every instance with the scene's shader: the picture is of the scene without shaders of their own
        i.shader = None
    w, h = (W, H) if name in ("mipped maps", "66 instances, 20 lights") else (LC.W, LC.H)
    return d, w, h, PICTURE_FRAMES.get(name, 1)


def frame_case(sample_data, name):
    """The GPU's P8 frames: a light_cases scene on small_sample, drawn with di_samples = 0 and max_lights = 16 at light_cases' 88 x 72."""
    d, _view, _frames = LC.make_case(MC.small_sample(sample_data), name)
    return d, dict(di_samples=0, max_lights=16)


def oracle_hits(data, rays):
    """The closest hits of `rays` by the oracle's walk, in RT64_RAY_HIT's layout: what the CPU tests hand the rule where the GPU tests hand it the device's."""
    import ray_rule
    from oracle import oracle_py
    o = oracle_py.OracleScene(data)
    try:
        o.render(W, H, images=False)
        return ray_rule.trace(o, rays)
    finally:
        o.close()
