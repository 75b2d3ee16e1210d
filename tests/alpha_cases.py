"""The scenes the alpha-honouring ray queries are checked on (tests/test_alpha_rule.py on the CPU, tests/test_gpu_alpha_query.py on the GPU).  TEST INFRASTRUCTURE.

Each case is (name, scene data, ray seed, device options, layer heights or None).  The scenes of tests/material_cases.py are reused; what is added stacks layers,
because random rays through the sample scene rarely cross more than one translucent surface: copies of the floor quad at several heights above the sphere, looked
at from above.  The rays are ray_rule.random_rays of the scene, 2000 per case, plus -- for the stacked cases -- 500 rays aimed steeply through the layers, a third
of them ending between two layers.  One vertex layout per scene (tests/material_rule.py): shaders with the alpha option read float4 inputs, shaders without it
float3, so the one scene that mixes them ("mixed") gives the former three inputs and the latter four -- 48 bytes either way.
"""
import numpy as np

import material_cases as MC
import ray_rule
from material_cases import IN1, IN3, IN4, OPT_ALPHA, OPT_EDGE, S0, TEX0, cc

RAYS, STEEP = 2000, 500
TILT = 0.05          # every layer leans this much (dy / dx), all the same way: a ray that starts inside a layer's world box (ray_rule.random_rays does that) does not start on its plane
FLOOR_MESH, FLOOR_INSTANCE = 3, 3
TEXEL_X_INPUT = cc((TEX0, S0, IN1, S0), (TEX0, S0, IN1, S0), OPT_ALPHA)
EDGE_SHADER = cc((TEX0, S0, IN1, S0), (TEX0, S0, IN1, S0), OPT_ALPHA | OPT_EDGE)
INPUT_ALPHA = cc((TEX0, S0, IN1, S0), (S0, S0, S0, IN1), OPT_ALPHA)                       # alpha = input alpha alone (>= 0.35): never cut out, not an edge shader
THREE_INPUTS = cc((TEX0, S0, IN1, S0), (TEX0, S0, IN3, S0), OPT_ALPHA)                   # "mixed": alpha = texel alpha x the third input's
NO_ALPHA_OPTION = cc((IN4, S0, TEX0, S0))                                                 # "mixed": no alpha option, four float3 inputs


def _plain_flags():
    from sm64rt_legacy_renderer_amd import rt64
    return rt64.SHADER_RASTER_ENABLED | rt64.SHADER_RAYTRACE_ENABLED                       # no normal or specular maps: alpha does not read them


def _from_above(d):
    """The camera 9 units above the origin, looking straight down (row-vector view matrix: the inverse of the camera's placement)."""
    c = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 9, 0, 1]], dtype=np.float64)
    d.view = np.linalg.inv(c).astype(np.float32)


def _layer(d, name, mesh, height, turn, diffuse, material, shader=None, scale=6.0, dx=0.0, dz=0.0):
    """A copy of the floor quad, `scale` times its size, turned by `turn` quarter turns about the vertical, leaning by TILT, at `height` above the origin; seen from both sides."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][turn % 4]
    t = np.array([[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0, 0, 0, 1]], dtype=np.float64) * scale
    t = t @ np.array([[1, TILT, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)          # world y rises with world x: the layer's box has a thickness
    t[3] = (dx, height, dz, 1.0)
    t = t.astype(np.float32)
    d.instances.append(sample_scene.InstanceData(name, mesh, t, t, diffuse, None, None, material, rt64.INSTANCE_DISABLE_BACKFACE_CULLING, shader=shader))


def _material(d, solid=1.0, shadow=1.0):
    from sm64rt_legacy_renderer_amd import sample_scene
    m = sample_scene.copy_material(d.instances[FLOOR_INSTANCE].material)
    m.solidAlphaMultiplier = solid; m.shadowAlphaMultiplier = shadow
    return m


def _base(sample_data, shader_id, seed):
    rng = np.random.default_rng(seed)
    d = MC.small_sample(sample_data)
    d.shader_id = shader_id; d.shader_flags = _plain_flags()
    d.meshes = [MC.relayout(m, shader_id, rng) for m in d.meshes]
    for k in (0, 4):          # texture_edge's ramps: alpha runs from 3 / 255 to 1 across the image
        img = d.textures[k].data.copy(); img[..., 3] = (np.arange(64) * 4 + 3)[None, :]
        d.textures[k] = MC._texture(d.textures[k].name + "_ramp", img)
    _from_above(d)
    return d, rng


VEIL_HEIGHTS = (3.4, 3.8, 4.2, 4.6, 5.0)
FENCE_HEIGHTS = (3.4, 4.0, 4.6)
MIXED_HEIGHTS = (3.4, 3.9, 4.4, 4.9)


def veils(sample_data):
    """The floor quad five more times above the sphere under an alpha-option shader (texel alpha x input alpha), shadowAlphaMultiplier 0.15 .. 0.4: a ray crosses
    two to five of them and then, perhaps, the sphere and the floor, so that sums land on both sides of 1."""
    d, _ = _base(sample_data, TEXEL_X_INPUT, 71)
    img = d.textures[4].data.copy(); img[..., 3] = 255
    d.textures[4] = MC._texture("tiles_dif_64_solid", img)
    for k, (h, mult, tex) in enumerate(zip(VEIL_HEIGHTS, (0.15, 0.2, 0.28, 0.34, 0.4), (4, 0, 4, 4, 0))):
        _layer(d, "veil%d" % k, FLOOR_MESH, h, k, tex, _material(d, 1.0, mult))
    return d


def fence(sample_data):
    """Three stacked texture-edge layers over the alpha-ramp textures, the middle one turned a quarter turn against the others so that the holes only partly line up, above the sphere (edge
    shader as well) and a floor that never cuts out: the closest accepted hit is often the second or third candidate, or the floor."""
    from sm64rt_legacy_renderer_amd import rt64
    d, _ = _base(sample_data, EDGE_SHADER, 72)
    for i in d.instances:
        i.material.solidAlphaMultiplier = 1.0; i.material.shadowAlphaMultiplier = 0.6
    d.instances[FLOOR_INSTANCE].shader = (INPUT_ALPHA, rt64.SHADER_FILTER_LINEAR, 0, 0, _plain_flags())
    for k, (h, tex, turn) in enumerate(zip(FENCE_HEIGHTS, (0, 4, 0), (1, 2, 1))):          # (top and bottom ramp the same way: about a quarter of the rays pass all three)
        _layer(d, "fence%d" % k, FLOOR_MESH, h, turn, tex, _material(d, 1.0, 0.6))
    return d


def mixed(sample_data):
    """K6's instances side by side under one veil: a layer whose shader has no alpha option and shadowAlphaMultiplier 0.5 (blocks fully; H10 alone would say
    0.5), a layer provably above 0.999 (input alpha 1, texel alpha 1, multiplier 1) and one of the same shader and mesh at 0.9 (subtracts 0.9)."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    d, rng = _base(sample_data, THREE_INPUTS, 73)
    img = d.textures[4].data.copy(); img[..., 3] = 255
    d.textures[4] = MC._texture("tiles_dif_64_solid", img)
    base = MC.small_sample(sample_data).meshes[FLOOR_MESH]
    d.meshes.append(MC.relayout(base, NO_ALPHA_OPTION, rng))                              # mesh 4: the floor quad as the shader without the alpha option reads it
    solid = MC.relayout(base, THREE_INPUTS, rng)
    v = solid.vertices.copy(); v["input3"][:, 3] = 1.0
    d.meshes.append(sample_scene.MeshData("floor_alpha_1", solid.flags, v, solid.indices))   # mesh 5: input alpha exactly 1
    flags = _plain_flags()
    _layer(d, "veil", FLOOR_MESH, MIXED_HEIGHTS[3], 1, 4, _material(d, 1.0, 0.3))
    _layer(d, "no alpha option", 4, MIXED_HEIGHTS[2], 0, 4, _material(d, 1.0, 0.5), shader=(NO_ALPHA_OPTION, rt64.SHADER_FILTER_LINEAR, 0, 0, flags), scale=2.5, dx=-4.0)
    _layer(d, "provably opaque", 5, MIXED_HEIGHTS[1], 0, 4, _material(d, 1.0, 1.0), scale=2.5, dx=4.0, dz=-2.0)
    _layer(d, "product 0.9", 5, MIXED_HEIGHTS[0], 2, 4, _material(d, 1.0, 0.9), scale=2.5, dx=1.0, dz=4.0)
    return d


def many_instances_with_edges(sample_data):
    """material_cases.many_instances (66 instances: the HBM walk, mixed combiners per wave) with a texture-edge shader on a third of the small spheres."""
    from sm64rt_legacy_renderer_amd import rt64
    d = MC.many_instances(sample_data)
    raster = rt64.SHADER_RASTER_ENABLED | rt64.SHADER_RAYTRACE_ENABLED
    for k, i in enumerate(d.instances[4:]):
        if k % 3 == 1:
            i.shader = (EDGE_SHADER, 0, 1, 1, raster)
            i.material.solidAlphaMultiplier = 0.8
    return d


def cases(sample_data):
    """The seeds are chosen so that the BVH walk and brute force enumerate the same intersections for every ray (tests/test_alpha_rule.py asserts it): the slab
    test of rule R2 widens tfar by a factor, which *narrows* it at negative t, so a walk drops a flat box -- the floor quad's -- behind the origin of a ray
    with a negative tMin where the triangle test alone would hit; with the seeds below no ray has such an intersection in its window."""
    return [("sample lds_cache=1", MC.small_sample(sample_data), 110, {"lds_cache": 1}, None),
            ("sample lds_cache=0", MC.small_sample(sample_data), 210, {"lds_cache": 0}, None),
            ("veils", veils(sample_data), 221, {}, VEIL_HEIGHTS),
            ("fence", fence(sample_data), 233, {}, FENCE_HEIGHTS),
            ("mixed", mixed(sample_data), 241, {}, MIXED_HEIGHTS),
            ("mipped fence", fence(sample_data), 253, {"generate_mipmaps": 1}, FENCE_HEIGHTS),
            ("66 instances, edge shader on a third", many_instances_with_edges(sample_data), 116, {"lds_cache": 1}, None),
            ("texture edge at 0.3 exactly", MC.texture_edge_on_the_threshold(sample_data), 270, {}, None)]


NAMES = ["sample lds_cache=1", "sample lds_cache=0", "veils", "fence", "mixed", "mipped fence", "66 instances, edge shader on a third", "texture edge at 0.3 exactly"]
STACKED_TRANSLUCENT, FENCES = ("veils", "mixed"), ("fence", "mipped fence")


def steep_rays(seed, heights, n=STEEP):
    """Rays aimed steeply through the layers: three quarters start above the top layer and go down, the others start under the floor and go up; directions of any
    length; every third ray ends between two neighbouring layers."""
    rng = np.random.default_rng(2000 + seed)
    down = np.arange(n) % 4 != 3
    o = np.zeros((n, 3)); d = np.zeros((n, 3))
    o[:, 0] = rng.uniform(-5.0, 5.0, n); o[:, 2] = rng.uniform(-5.0, 5.0, n)
    o[:, 1] = np.where(down, max(heights) + rng.uniform(0.2, 1.0, n), -rng.uniform(0.5, 1.5, n))
    d[:, 0] = rng.normal(0.0, 0.2, n); d[:, 2] = rng.normal(0.0, 0.2, n); d[:, 1] = np.where(down, -1.0, 1.0)
    d *= (10.0 ** rng.uniform(-1.0, 1.0, n))[:, None]
    tmax = np.full(n, np.inf)
    ends = np.arange(n) % 3 == 0
    k = rng.integers(0, len(heights) - 1, n)
    h = np.asarray(heights)
    y_end = h[k] + rng.uniform(0.2, 0.8, n) * (h[k + 1] - h[k])
    tmax[ends] = (np.abs(y_end - o[:, 1]) / np.abs(d[:, 1]))[ends]
    r = np.zeros((n, 8), dtype=np.float32)
    r[:, 0:3] = o; r[:, 4:7] = d; r[:, 7] = tmax
    return r


def rays_of(data, seed, heights):
    rays = ray_rule.random_rays(data, seed, RAYS, floor_instance=FLOOR_INSTANCE)
    if heights is not None:
        rays = np.ascontiguousarray(np.concatenate([rays, steep_rays(seed, heights)]))
    return rays


def lods_of(seed, n, options):
    return MC.lods(seed, n, MC.mipmapped(options))
