"""CPU guard of the saturated hit-list scenes that tests/test_gpu_kbuffer.py renders on the GPU: K parallel translucent sheets above the camera, between the
floor and the light, so that every surface ray that crosses the stack -- primary rays into the upper half of the view, GI, mirror and shadow rays from the
floor -- collects more hits than the 16 + 1 slots of the per-pixel list (rt64_shader.cpp:553-580).  The oracle alone, no GPU: a change of the scene
geometry must not quietly drop the GPU tests below 16 hits.

The scene builder lives here so that both modules render the same sheets.
"""
import copy

import numpy as np
import pytest

from oracle import oracle_py

W, H = 320, 180
MAX_HIT_QUERIES = 16
ALPHA = 0.1                         # solidAlphaMultiplier of a sheet: layer 17 weighs 0.9^16 * 0.1 = 0.0185 of its colour
BOTTOM, SPACING = 2.3, 0.035        # sheet k lies at y = BOTTOM + k * SPACING at z = Z1 (the camera is at y = 2): the first 16 sheets of every K are the same 16
SLOPE = 0.004                       # ... and rises by SLOPE per unit towards -z: parallel planes whose boxes overlap their neighbours'
X0, X1, Z1 = -40.0, 40.0, 9.9
Z0_LONG, Z0_SHORT = -60.0, -15.0    # even sheets reach z = -60, odd ones z = -15: a long sheet's box is entered before the short sheets above it are hit,
                                    # so hits do not arrive nearest first and nearer ones keep pushing the farthest entry into slot 16
LAYOUTS = ("instances", "one_mesh", "depth_bias", "ignored_hits")
S0, IN1, TEX0 = 0, 1, 5
OPT_ALPHA, OPT_EDGE = 1 << 24, 1 << 26


def _cc(color, alpha, opts):
    v = 0
    for i, c in enumerate(color):
        v |= c << (3 * i)
    for i, c in enumerate(alpha):
        v |= c << (12 + 3 * i)
    return v | opts


# colour = texel x vertex colour, alpha = vertex alpha: the sample's vertex layout (position, normal, uv, input1 rgba) and, with the floor's
# input1 = 1, the sample's floor; the sheets' vertex colours tell them apart in every layout, one mesh included
SHADER_ID = _cc((TEX0, S0, IN1, S0), (S0, S0, S0, IN1), OPT_ALPHA)
EDGE_SHADER_ID = SHADER_ID | OPT_EDGE


def sheet_colour(k):
    a = 2.1 * k
    return (0.5 + 0.5 * np.sin(a), 0.5 + 0.5 * np.sin(a + 2.1), 0.5 + 0.5 * np.sin(a + 4.2))


def sheet_height(k):
    return BOTTOM + k * SPACING


def sheet_z0(k):
    return Z0_SHORT if k % 2 else Z0_LONG


def depth_bias(k):
    """Layout "depth_bias": 0, 0.12 or 0.24 -- neighbouring sheets are 0.035 / sin(angle) >= 0.09 apart along a primary ray, so the sort key
    t - depthBias orders some pairs against their t order."""
    return 0.12 * ((5 * k) % 3)


def edge_sheet(K):
    """Layout "ignored_hits": the texture-edge sheet, second from the top (its opaque half hides only the last sheet and the sky)."""
    return K - 2


def faces_up(k):
    """Layout "ignored_hits": every third sheet turns its back to the camera and the floor -- rays from below skip it (back-face culling) ..."""
    return k % 3 == 1


def cull_disabled(k):
    """... unless it is flagged DISABLE_BACKFACE_CULLING, every other one of them."""
    return k % 6 == 1


def _sheet_vertices(k, edge=False):
    from sm64rt_legacy_renderer_amd import sample_scene
    v = np.zeros(4, dtype=sample_scene.VERTEX_DTYPE)
    y0, z0 = sheet_height(k), sheet_z0(k)
    y1 = y0 + SLOPE * (Z1 - z0)
    v["position"] = [(X0, y1, z0, 1.0), (X1, y1, z0, 1.0), (X0, y0, Z1, 1.0), (X1, y0, Z1, 1.0)]
    v["uv"] = [(0.0, 0.0), (8.0, 0.0), (0.0, 8.0), (8.0, 8.0)]
    v["normal"] = (0.0, 1.0, 0.0)
    v["input1"][:, :3] = sheet_colour(k)
    v["input1"][:, 3] = (0.0, 1.0, 1.0, 0.0) if edge else 1.0      # edge: alpha across the sheet, IgnoreHit() where alpha <= 0.3 (rt64_shader.cpp:502-511)
    return v


SHEET_IDX = np.array([0, 1, 2, 3, 2, 1], dtype=np.uint32)        # against the floor's winding: front faces look down, at the camera and the floor
SHEET_IDX_UP = np.array([2, 1, 0, 1, 2, 3], dtype=np.uint32)


def kbuffer_scene(sample_data, K, layout="instances", mutate=None):
    """The sample scene without its sphere, with K sheets (sheet 0 nearest the camera) above the camera.  Instance order: HUD, floor, then the sheets.
    Returns SceneData with two more attributes: `floor_instance` (the sheets' instances follow it, sheet 0 first) and `edge_instance`, the index of the
    texture-edge instance (layout "ignored_hits") or None."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    assert layout in LAYOUTS
    d = copy.copy(sample_data)
    d.shader_id = SHADER_ID
    floor = next(i for i in sample_data.instances if i.name == "floor")
    hud = [i for i in sample_data.instances if i.name.startswith("hud")]
    d.meshes = [copy.copy(m) for m in sample_data.meshes]
    d.instances = [copy.copy(i) for i in hud] + [copy.copy(floor)]
    for i in d.instances:
        i.material = sample_scene.copy_material(i.material)
    ident = np.eye(4, dtype=np.float32)
    edge = edge_sheet(K) if layout == "ignored_hits" else None
    d.edge_instance = None
    d.floor_instance = len(d.instances) - 1                           # the sheets follow it

    def material(k):
        m = sample_scene.copy_material(floor.material)
        m.solidAlphaMultiplier = 1.0 if k == edge else ALPHA
        if layout == "depth_bias":
            m.depthBias = depth_bias(k)
        return m

    def flags(k):
        return rt64.INSTANCE_DISABLE_BACKFACE_CULLING if layout == "ignored_hits" and cull_disabled(k) else 0

    def indices(k):
        return SHEET_IDX_UP if layout == "ignored_hits" and faces_up(k) else SHEET_IDX

    if layout == "one_mesh":
        v = np.concatenate([_sheet_vertices(k) for k in range(K)])
        idx = np.concatenate([SHEET_IDX + 4 * k for k in range(K)]).astype(np.uint32)
        d.meshes.append(sample_scene.MeshData("sheets", rt64.MESH_RAYTRACE_ENABLED, v, idx))
        d.instances.append(sample_scene.InstanceData("sheets", len(d.meshes) - 1, ident, ident, floor.diffuse, None, None, material(0), flags(0)))
    else:
        for k in range(K):
            d.meshes.append(sample_scene.MeshData("sheet%d" % k, rt64.MESH_RAYTRACE_ENABLED, _sheet_vertices(k, edge=(k == edge)), indices(k)))
            d.instances.append(sample_scene.InstanceData("sheet%d" % k, len(d.meshes) - 1, ident, ident, floor.diffuse, None, None, material(k), flags(k)))
            if k == edge:
                d.edge_instance = len(d.instances) - 1
    if mutate:
        mutate(d)
    return d


def set_edge_shader_oracle(o, data):
    """The oracle's side of the one texture-edge instance (its own shader id; the rest of the scene keeps SHADER_ID)."""
    if data.edge_instance is None:
        return
    import ctypes as C
    desc = o._desc(data.instances[data.edge_instance])
    desc.shaderId = EDGE_SHADER_ID
    o.L.oracle_scene_set_instance(o.scene, data.edge_instance, C.byref(desc))


def crosses_stack(o, d, K, margin=0.25):
    """Rays (origins o [..., 3], directions d [..., 3]) that cross every one of the K sheets inside its rectangle."""
    den = d[..., 1] + SLOPE * d[..., 2]                           # plane y = y0 + SLOPE (Z1 - z) along the ray
    ok = np.abs(den) > 1e-4
    for k in range(K):
        t = np.where(ok, (sheet_height(k) + SLOPE * (Z1 - o[..., 2]) - o[..., 1]) / np.where(ok, den, 1.0), 0.0)
        x, z = o[..., 0] + t * d[..., 0], o[..., 2] + t * d[..., 2]
        ok &= (t > 0.2) & (x > X0 + margin) & (x < X1 - margin) & (z > sheet_z0(k) + margin) & (z < Z1 - margin)
    return ok


def _camera(data):
    return np.linalg.inv(data.view.astype(np.float64))[3, :3]


def covered_mask(ref, data, K):
    """Pixels whose primary ray crosses the whole stack (from the view-direction image of an oracle frame without mirrors)."""
    d = ref["viewDirection"][..., :3].astype(np.float64)
    return crosses_stack(np.broadcast_to(_camera(data), d.shape), d, K)


def floor_ray_mask(ref, data, K, kind):
    """(`ref`: a frame without mirrors -- a reflection pass rewrites the view-direction image.)
    Floor pixels whose mirror ray (kind "mirror") or shadow ray towards the scene's one light (kind "shadow") crosses the whole stack."""
    cam = _camera(data)
    d = ref["viewDirection"][..., :3].astype(np.float64)
    floor_rt = data.floor_instance - sum(1 for i in data.instances[:data.floor_instance] if i.name.startswith("hud"))      # index among the ray-traced instances
    on_floor = (ref["primaryHit"][..., 3] != 0xFFFFFFFF) & (ref["primaryHit"][..., 3] >> 24 == floor_rt)
    t = np.where(d[..., 1] < -1e-3, -cam[1] / np.where(d[..., 1] < -1e-3, d[..., 1], -1.0), 0.0)
    p = cam + t[..., None] * d
    if kind == "mirror":
        r = d * (1.0, -1.0, 1.0)
    else:
        lp = data.lights[0].position
        r = np.array([lp.x, lp.y, lp.z]) - p
        r /= np.linalg.norm(r, axis=-1, keepdims=True)
    return on_floor & crosses_stack(p, r, K)


def render_oracle(data, **kw):
    o = oracle_py.OracleScene(data)
    try:
        set_edge_shader_oracle(o, data)
        return o.render(W, H, **kw)
    finally:
        o.close()


LAYER_WEIGHT = (1.0 - ALPHA) ** MAX_HIT_QUERIES * ALPHA             # weight of the entry in slot 16: 0.0185
LIT_MAX = 2.0                                                        # a unit texel x vertex colour lit by the sample's light + ambient + eye light stays below 2


@pytest.fixture(scope="module")
def frames(sample_data, oracle_lib):
    out = {}
    for layout in LAYOUTS:
        for K in (15, 16, 40):
            d = kbuffer_scene(sample_data, K, layout)
            r = render_oracle(d)
            out[layout, K] = (r, covered_mask(r, d, K))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_stack_covers_a_large_part_of_the_view(frames, layout):
    for K in (15, 16, 40):
        r, m = frames[layout, K]
        assert m.mean() > 0.4, (K, float(m.mean()))                  # 24 320 of 57 600 pixels at K = 40
        # every covered primary ray tests at least one triangle per sheet it collects (the oracle reports totals: a lower bound, not a per-ray count)
        assert r["counters"]["trianglesTestedPrimary"] >= min(K, MAX_HIT_QUERIES) * int(m.sum())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sixteen_layers_all_reach_the_picture(frames, layout):
    """K = 15 -> 16: the 16th sheet changes every covered pixel, so the list is not cut before its 16 entries."""
    (a, ma), (b, mb) = frames[layout, 15], frames[layout, 16]
    m = ma & mb
    d = np.abs(a["output"][..., :3] - b["output"][..., :3]).max(axis=-1)[m]
    assert d.min() > 2e-3, float(d.min())


@pytest.mark.parametrize("layout", ("instances", "one_mesh", "depth_bias"))
def test_layers_behind_the_list_weigh_at_most_one_slot(frames, layout):
    """K = 16 -> 40 with the 24 extra sheets behind the first 16: the list saturates -- at most the entry in slot 16 joins the picture, one layer's
    weight (0.9^16 x 0.1 x colour).  An unbounded list would composite 24 more layers over the floor, about 0.17 of the colour.  (Layout "ignored_hits" moves
    its opaque texture-edge sheet from inside the list at K = 16 to behind it at K = 40: not one layer apart.)"""
    (a, ma), (b, mb) = frames[layout, 16], frames[layout, 40]
    m = ma & mb
    assert m.sum() > 20000
    d = np.abs(a["output"][..., :3] - b["output"][..., :3]).max(axis=-1)[m]
    assert d.max() <= LAYER_WEIGHT * LIT_MAX + 1e-4, float(d.max())
    assert (d > 1e-4).mean() > 0.95                                  # ... and slot 16 is filled: the list really runs over
