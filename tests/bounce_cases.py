"""The scenes the bounce records and mirror chains are checked on (tests/test_bounce_rule.py on the CPU, tests/test_gpu_bounce_query.py on the GPU).  TEST INFRASTRUCTURE.

Each case is (scene data, ray seed, device options, ray flags).  Five are mirror_cases.make_case's scenes -- mirrors that face each other, glass at grazing
incidence, translucent back faces, a textured mirror -- built on material_cases.small_sample, whose textures are small RGBA8 images the material rule can read.
Four are added: the sample's normal maps on mirrors under generated mip chains with one lod per ray, instances with a depth bias, a sphere without back-face
culling hit from inside under RT64_RAY_FLAG_CULL_BACK_FACING, and alpha_cases' texture-edge fence over a mirror floor.
The rays: 1500 of ray_rule.random_rays (any origin, any direction of any length, grazing, from inside boxes, narrow windows: about half of them miss) and 500
aimed at points of the scene's instances from outside, a tenth of those turned away so that they miss; per case, where a share needs them, rays aimed at one
instance from a chosen side.
"""
import numpy as np

import alpha_cases as AC
import lighting_cases
import material_cases as MC
import mirror_cases as MRC
import ray_rule

FROM_MIRROR_CASES = ("floor", "facing", "glass", "translucent", "textured")
NAMES = FROM_MIRROR_CASES + ("mapped mirrors", "depth bias", "from behind", "fence over a mirror")
SEEDS = {name: 501 + k for k, name in enumerate(NAMES)}
RANDOM, AIMED = 1500, 500

# What makes a case worth running, as shares of its real hits measured on the rule: at least this much (mirror hits, glass hits, total-internal hits, back
# faces, mapped normals).  Set well under what the geometry gives -- the floor is a mirror in every case but "glass" and takes a third of the hits or more; the
# aimed rays of "glass" meet the slab under 40 degrees of elevation, where a factor of 1.5 reflects totally; a ray from inside a closed sphere can only leave
# through a back face -- so that a reseeded batch still passes, and above what a broken case (no mirror, a slab nobody hits) would show.
SHARES = {
    "floor": (0.25, 0.0, 0.0, 0.05, 0.0), "facing": (0.40, 0.0, 0.0, 0.05, 0.0), "glass": (0.0, 0.25, 0.05, 0.05, 0.0), "translucent": (0.40, 0.0, 0.0, 0.10, 0.0),
    "textured": (0.25, 0.0, 0.0, 0.05, 0.0), "mapped mirrors": (0.60, 0.15, 0.0, 0.05, 0.60), "depth bias": (0.25, 0.0, 0.0, 0.05, 0.0),
    "from behind": (0.40, 0.15, 0.0, 0.20, 0.40), "fence over a mirror": (0.10, 0.0, 0.0, 0.05, 0.0),
}
UNDECIDED_CAP = lighting_cases.UNDECIDED_CAP          # 2 % of a case's real hits

# the case built to catch each wrong variant of the rule
MUTATION_CASE = {
    "direction_normalised": "floor", "geometric_normal": "mapped mirrors", "back_normal_not_turned": "from behind", "no_depth_bias": "depth bias",
    "a4_position": "depth bias", "eta_inverted": "glass", "tir_ignored": "glass", "fresnel_no_floor": "facing", "fresnel_on_non_mirror": "glass", "tmin_zero": "floor",
}


def _named(d, name):
    return next(i for i in d.instances if i.name == name)


def _from_mirror(sample_data, name):
    return MRC.make_case(MC.small_sample(sample_data), name)["data_at"](0)


def make_case(sample_data, name):
    """-> (SceneData, seed, device options, ray flags)."""
    from sm64rt_legacy_renderer_amd import rt64
    seed = SEEDS[name]
    if name in FROM_MIRROR_CASES:
        return _from_mirror(sample_data, name), seed, {}, 0
    if name == "mapped mirrors":
        d = MC.detail_scales(sample_data)
        sphere, floor = _named(d, "sphere"), _named(d, "floor")
        sphere.material.reflectionFactor = 0.2; sphere.material.reflectionFresnelFactor = 1.0; sphere.material.refractionFactor = 0.8
        floor.material.reflectionFactor = 0.4; floor.material.reflectionFresnelFactor = 0.5
        return d, seed, {"generate_mipmaps": 1}, 0
    if name == "depth bias":
        d = _from_mirror(sample_data, "floor")
        _named(d, "floor").material.depthBias = 0.25; _named(d, "sphere").material.depthBias = -0.125
        _named(d, "sphere").material.reflectionFactor = 0.1
        return d, seed, {}, 0
    if name == "from behind":
        d = MC.inside_sphere(sample_data)
        sphere, floor = _named(d, "sphere"), _named(d, "floor")
        sphere.material.reflectionFactor = 0.3; sphere.material.reflectionFresnelFactor = 1.5; sphere.material.refractionFactor = 1.25
        floor.material.reflectionFactor = 0.5; floor.material.reflectionFresnelFactor = 0.5
        return d, seed, {}, ray_rule.CULL_BACK_FACING
    if name == "fence over a mirror":
        d = AC.fence(sample_data)
        floor = d.instances[AC.FLOOR_INSTANCE]
        floor.material.reflectionFactor = 0.5; floor.material.reflectionFresnelFactor = 1.0
        return d, seed, {}, 0
    raise KeyError(name)


def _world(data, inst):
    p = data.meshes[inst.mesh].vertices["position"][:, :3].astype(np.float64)
    t = np.asarray(inst.transform, dtype=np.float64)
    return p @ t[:3, :3] + t[3, :3]


def _pack(o, d):
    r = np.zeros((len(o), 8), dtype=np.float32)
    r[:, 0:3] = o; r[:, 4:7] = d; r[:, 7] = np.inf
    return r


def aimed_rays(data, rng, n, instances=None, elevation=(-1.0, 1.0), inside=False):
    """n rays towards points of the instances' vertices' boxes (every ray-traced instance, or those named), from 6 to 12 units away in a direction whose sine of
    elevation is drawn from `elevation` (inside: from the middle of the box outwards instead), with directions of length 0.25 to 4; every tenth turned round."""
    inst = [i for i in data.instances if (instances is None or i.name in instances) and data.meshes[i.mesh].flags & 1]
    pick = rng.integers(len(inst), size=n)
    lo = np.array([_world(data, i).min(axis=0) for i in inst])[pick]; hi = np.array([_world(data, i).max(axis=0) for i in inst])[pick]
    target = lo + (hi - lo) * rng.uniform(0.1, 0.9, size=(n, 3))
    s = rng.uniform(elevation[0], elevation[1], size=n); phi = rng.uniform(0.0, 2.0 * np.pi, size=n)
    c = np.sqrt(1.0 - s * s)
    away = np.stack([c * np.cos(phi), s, c * np.sin(phi)], axis=1)
    if inside:
        origin = 0.5 * (lo + hi) + (hi - lo) * rng.uniform(-0.1, 0.1, size=(n, 3))
        d = away
    else:
        origin = target + away * rng.uniform(6.0, 12.0, size=(n, 1))
        d = target - origin
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d * rng.uniform(0.25, 4.0, size=(n, 1))
    d[::10] *= -1.0 if not inside else 1.0
    return _pack(origin, d)


def rays_and_lods(data, name, seed, options):
    floor = next(k for k, i in enumerate(data.instances) if i.name == "floor")
    rng = np.random.default_rng(7000 + seed)
    parts = [ray_rule.random_rays(data, seed, RANDOM, floor_instance=floor)]
    if name == "glass":          # the slab under 8 to 40 degrees of elevation (total internal reflection at 1.5), the sphere from anywhere
        parts += [aimed_rays(data, rng, 250, ("slab",), (0.14, 0.64)), aimed_rays(data, rng, 250, ("sphere",))]
    elif name == "from behind":
        parts += [aimed_rays(data, rng, 300, ("sphere",), inside=True), aimed_rays(data, rng, 200)]
    elif name == "fence over a mirror":
        parts += [AC.steep_rays(seed, AC.FENCE_HEIGHTS)[:AIMED]]
    else:
        parts += [aimed_rays(data, rng, AIMED)]
    rays = np.ascontiguousarray(np.concatenate(parts).astype(np.float32))
    lods = MC.lods(seed, len(rays), True) if MC.mipmapped(options) else None
    return rays, lods


def oracle_hits(data, rays, flags=0):
    """The closest hits of `rays` by the oracle's walk, in RT64_RAY_HIT's layout: what the CPU tests hand the rule where the GPU tests hand it the device's."""
    from oracle import oracle_py
    o = oracle_py.OracleScene(data)
    try:
        o.render(lighting_cases.W, lighting_cases.H, images=False)
        return ray_rule.trace(o, rays, flags)
    finally:
        o.close()
