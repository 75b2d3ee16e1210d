"""Scenes and rays of the layered ray queries (rules T1-T12), shared by tests/test_layers_rule.py (CPU, the rule alone) and tests/test_gpu_layers_query.py.
TEST INFRASTRUCTURE.

The sheet stacks are `test_oracle_kbuffer.kbuffer_scene`'s -- K translucent sheets above the camera, over the sample scene's floor -- with the sheets' solid alpha
multipliers set to 0.2, 0.4 and 0.6 in turn (51, 102 and 153 of 255: exact UNORM8 steps; that module's own 0.1 is 25.5 of 255, a rounding boundary, and would leave
every weight undecided).  K = 3 and 8 give lists of class (a) of T5, K = 20 class (b) -- every layout but "depth_bias" -- and class (c).  The case "decal" adds what
the stacks lack: an opaque decal 0.02 under the floor whose depthBias of 0.1 sorts it in front of the floor, a glass sheet of alpha 0.25 (not a UNORM8 step) on top
of the stack, and under ten sheets of alpha 0.6 a sheet of alpha 1 / 255, whose weight of 0.4^10 / 255 = 4.1e-7 the frame skips.
"""
import copy

import numpy as np

import test_oracle_kbuffer as KB

MULTIPLIERS = (0.2, 0.4, 0.6)
W, H = 64, 36
# name -> (K, layout, the classes of T5 the case is meant for)
STACKS = {"%s_%d" % (layout, K): (K, layout, "a" if K < 16 else "c" if layout == "depth_bias" else "b") for K in (3, 8, 20) for layout in KB.LAYOUTS}
NAMES = tuple(sorted(STACKS)) + ("decal",)
DECAL_K = 13
FAINT, GLASS = 10, 12          # sheets of the decal case: 0..9 alpha 0.6, 10 alpha 1 / 255, 11 alpha 0.6, 12 the glass sheet of alpha 0.25


def _own_edge_shader(d):
    if d.edge_instance is not None:          # Rt64Scene and material_rule read an instance's own shader from `shader`; the oracle only enumerates and needs none
        d.instances[d.edge_instance].shader = (KB.EDGE_SHADER_ID, d.shader_filter, d.shader_haddr, d.shader_vaddr, d.shader_flags)


def stack_case(sample_data, K, layout):
    def mutate(d):
        for k, inst in enumerate(d.instances[d.floor_instance + 1:]):
            if d.edge_instance is None or d.floor_instance + 1 + k != d.edge_instance:
                inst.material.solidAlphaMultiplier = MULTIPLIERS[k % 3]
        _own_edge_shader(d)
    return KB.kbuffer_scene(sample_data, K, layout, mutate=mutate)


def decal_case(sample_data):
    from sm64rt_legacy_renderer_amd import sample_scene

    def mutate(d):
        sheets = d.instances[d.floor_instance + 1:]
        for k, inst in enumerate(sheets):
            inst.material.solidAlphaMultiplier = 0.6
        sheets[FAINT].material.solidAlphaMultiplier = 1.0 / 255.0
        sheets[GLASS].material.solidAlphaMultiplier = 0.25
        sheets[GLASS].material.refractionFactor = 1.3
        floor = d.instances[d.floor_instance]
        t = np.array(floor.transform, dtype=np.float32).copy()
        t[:3, :3] *= 0.4; t[3, 1] -= 0.02
        m = sample_scene.copy_material(floor.material)
        m.depthBias = 0.1
        d.instances.append(sample_scene.InstanceData("decal", floor.mesh, t, t.copy(), floor.diffuse, floor.normal, floor.specular, m, floor.flags))
    return KB.kbuffer_scene(sample_data, DECAL_K, "instances", mutate=mutate)


def case(sample_data, name):
    """-> (SceneData, number of sheets, classes meant)"""
    if name == "decal":
        return decal_case(sample_data), DECAL_K, "a"
    K, layout, classes = STACKS[name]
    return stack_case(sample_data, K, layout), K, classes


def rays_of(K, seed, per_kind=56):
    """A few hundred seeded rays, (N, 8) float32: down through the stack onto the floor, up from under it, grazing the sheets' edges, from inside the stack, with
    short windows that cut it, and Q6-invalid ones."""
    rng = np.random.default_rng(seed)
    m = per_kind
    top = KB.sheet_height(K - 1) + KB.SLOPE * 80.0
    out = []

    def pack(o, d, tmin, tmax):
        r = np.zeros((len(o), 8), dtype=np.float32)
        r[:, 0:3] = o; r[:, 3] = tmin; r[:, 4:7] = d; r[:, 7] = tmax
        return r

    def around(y0, y1, k, spread=9.0):
        o = rng.uniform((-spread, y0, -spread), (spread, y1, spread), size=(k, 3))
        return o
    scale = 10.0 ** rng.uniform(-0.5, 0.5, size=(m, 1))
    # 1. down through the stack: steep and slanted
    d = np.concatenate([rng.uniform(-0.6, 0.6, size=(m, 1)), -np.ones((m, 1)), rng.uniform(-0.6, 0.6, size=(m, 1))], axis=1) * scale
    out.append(pack(around(top + 0.5, top + 2.0, m), d, 0.0, 1000.0))
    # 2. up from under the stack
    d = np.concatenate([rng.uniform(-0.8, 0.8, size=(m, 1)), np.ones((m, 1)), rng.uniform(-0.8, 0.8, size=(m, 1))], axis=1) * scale
    out.append(pack(around(0.5, 2.2, m), d, 0.0, 1000.0))
    # 3. grazing the sheets' edges: across x = X1 and across the short sheets' far edge z = Z0_SHORT
    k = m // 2
    o = np.stack([np.full(k, KB.X1 - 0.5) + rng.uniform(-0.4, 0.4, size=k), np.full(k, 1.8), rng.uniform(-10, 5, size=k)], axis=1)
    d = np.stack([rng.uniform(-0.3, 0.3, size=k), np.ones(k), rng.uniform(-0.1, 0.1, size=k)], axis=1)
    out.append(pack(o, d, 0.0, 1000.0))
    o = np.stack([rng.uniform(-10, 10, size=m - k), np.full(m - k, 1.8), np.full(m - k, KB.Z0_SHORT + 0.5) + rng.uniform(-0.4, 0.4, size=m - k)], axis=1)
    d = np.stack([rng.uniform(-0.1, 0.1, size=m - k), np.ones(m - k), rng.uniform(-0.3, 0.3, size=m - k)], axis=1)
    out.append(pack(o, d, 0.0, 1000.0))
    # 4. from inside the stack, either way
    d = np.concatenate([rng.uniform(-0.5, 0.5, size=(m, 1)), rng.choice([-1.0, 1.0], size=(m, 1)), rng.uniform(-0.5, 0.5, size=(m, 1))], axis=1)
    out.append(pack(around(KB.sheet_height(0), KB.sheet_height(K - 1) + 0.05, m, 5.0), d, 0.0, 1000.0))
    # 5. short windows that cut the stack: from above, the window ends inside it or just behind it
    d = np.concatenate([rng.uniform(-0.3, 0.3, size=(m, 1)), -np.ones((m, 1)), rng.uniform(-0.3, 0.3, size=(m, 1))], axis=1)
    o = around(top + 0.5, top + 1.0, m)
    depth = (o[:, 1] - KB.sheet_height(0)) * rng.uniform(0.3, 1.3, size=m)
    out.append(pack(o, d, rng.uniform(0.0, 0.6, size=m), depth))
    # 6. Q6-invalid
    bad = pack(around(3.5, 4.0, 8), np.tile([[0.1, -1.0, 0.1]], (8, 1)), 0.0, 1000.0)
    bad[0, 0] = np.nan; bad[1, 5] = np.inf; bad[2, 4:7] = 0.0; bad[3, 3] = 5.0; bad[3, 7] = 5.0; bad[4, 3] = 9.0; bad[4, 7] = 2.0; bad[5, 7] = np.nan; bad[6, 1] = -np.inf; bad[7, 3] = np.nan
    out.append(bad)
    return np.ascontiguousarray(np.concatenate(out).astype(np.float32))


def enumerate_candidates(data, rays, cull=False):
    """-> (OracleScene, candidates): the oracle scene stays open for the ordered walks of class (c); close it."""
    from oracle import oracle_py
    import alpha_rule
    o = oracle_py.OracleScene(data)
    o.render(W, H, images=False)
    return o, alpha_rule.candidates(o, rays, cull=cull)
