"""The surface-record rule (tests/surface_rule.py, rules A1-A8 of DESIGN.md 4) checked on the CPU: hits come from the oracle's traversal (tests/ray_rule.py).

 * convention tie: the rule's position is origin + t direction, so barycentrics, vertex order, triangle numbering and instance numbering are the traversal's;
 * the geometric normal is perpendicular to the triangle's world-space edges, and agrees in side with the unflipped shading normal on the smooth sphere;
 * the bound is not vacuous: at most 1e-4 of the scene's extent / of 1 / of the largest |uv| on every case;
 * every wrong variant (`mutate=`) leaves the bound on at least one named case -- the counts measured here are recorded in MUTATION_MISSES;
 * at most 1 % of the hits are undecided in every case.
"""
import numpy as np
import pytest

import ray_rule
import surface_cases
import surface_rule as S

W, H = 64, 36
# hits outside the bound per mutation on the case named (of the hits of surface_cases.RAYS rays; the assertion is "at least one", the figures are what was seen)
MUTATION_CASES = {
    "uv_swapped": "sample lds_cache=1",
    "b0_on_p1": "sample lds_cache=1",
    "normal_by_object_to_world": "rotation x scale (1, .5, 2)",
    "no_flip": "sample lds_cache=1",
    "flip_geometric": "sample lds_cache=1",
    "no_zero_fallback": "zero vertex normals",
    "no_renormalise": "sample lds_cache=1",
}
MUTATION_MISSES = {"uv_swapped": 443, "b0_on_p1": 443, "normal_by_object_to_world": 174, "no_flip": 208, "flip_geometric": 208, "no_zero_fallback": 196, "no_renormalise": 253}


@pytest.fixture(scope="module")
def solved(sample_data, oracle_lib):
    """name -> (data, rays, hits, rule): one oracle traversal and one evaluation of the rule per case, shared by the tests below and left unchanged."""
    from oracle import oracle_py
    out = {}
    for name, data, seed, _options in surface_cases.cases(sample_data, with_random=False):
        o = oracle_py.OracleScene(data)
        try:
            o.render(W, H, images=False)
            rays = ray_rule.random_rays(data, seed, surface_cases.RAYS, floor_instance=3)
            hits = ray_rule.trace(o, rays)
        finally:
            o.close()
        out[name] = (data, rays, hits, S.surfaces(data, rays, hits))
    return out


def test_instance_numbering_is_the_raytraced_instances_in_creation_order(sample_data):
    assert S.raytraced_instances(sample_data) == [1, 3]
    assert S.vertex_layout(sample_data.shader_id) == {"normal": 16, "uv": 28, "has_uv": True, "size": 52}
    assert S.vertex_layout(surface_cases.NO_UV_SHADER) == {"normal": 16, "uv": 28, "has_uv": False, "size": 40}


def test_position_is_origin_plus_t_direction(solved):
    for name, (data, rays, hits, rule) in solved.items():
        real = rule["kind"] == 2
        assert real.sum() > surface_cases.RAYS // 20, name
        assert np.array_equal(real, hits.view(np.int32)[:, 3] >= 0), name           # the oracle's hits are all in range
        o, d, t = rays[real, 0:3].astype(np.float64), rays[real, 4:7].astype(np.float64), hits[real, 0].astype(np.float64)
        along = o + t[:, None] * d
        scale = np.maximum(np.maximum(np.abs(o).max(axis=1), np.abs(along).max(axis=1)), np.abs(t[:, None] * d).max(axis=1))
        miss = np.abs(rule["position"][0][real] - along).max(axis=1) / scale
        print("%-28s convention tie: max %.2e of the largest coordinate, %d hits" % (name, miss.max(), real.sum()))
        assert miss.max() < 1e-4, (name, miss.max())


def test_geometric_normal_is_perpendicular_to_the_world_space_edges(solved):
    for name, (data, rays, hits, rule) in solved.items():
        rt = S.raytraced_instances(data)
        real = np.nonzero(rule["kind"] == 2)[0]
        layout = S.vertex_layout(data.shader_id)
        for k, index in enumerate(rt):
            sel = real[rule["instance"][real] == k]
            if not len(sel):
                continue
            inst = data.instances[index]; mesh = data.meshes[inst.mesh]
            T = np.asarray(inst.transform, dtype=np.float64)
            corner = [np.asarray(mesh.indices, dtype=np.int64)[3 * rule["primitive"][sel] + c] for c in range(3)]
            pw = [S._fetch(mesh, layout, corner[c], 0, 3) @ T[:3, :3] + T[3, :3] for c in range(3)]
            g = rule["geometric"][0][sel]
            assert np.allclose(np.linalg.norm(g, axis=1), 1.0, atol=1e-6), name
            for e in (pw[1] - pw[0], pw[2] - pw[0]):
                cosine = np.abs((g * e).sum(axis=1)) / np.linalg.norm(e, axis=1)
                assert cosine.max() < 1e-5, (name, k, cosine.max())
        if "zero" not in name:
            # the sphere is smooth: its shading normal, flip undone, lies on the geometric normal's side
            sph = real[rule["instance"][real] == 0]
            sign = np.where(rule["back"][sph], -1.0, 1.0)[:, None]
            assert ((rule["geometric"][0][sph] * rule["shading"][0][sph] * sign).sum(axis=1) > 0.0).all(), name


def test_the_bound_is_not_vacuous(solved):
    for name, (data, rays, hits, rule) in solved.items():
        real = rule["kind"] == 2
        lo, hi = ray_rule.scene_bounds(data)
        extent = float((hi - lo).max())
        pos, nrm = rule["position"][1][real].max(), max(rule["geometric"][1][real].max(), rule["shading"][1][real].max())
        print("%-28s bounds: position %.2e (extent %.1f), normal %.2e, uv %.2e" % (name, pos, extent, nrm, rule["uv"][1][real].max()))
        assert pos <= 1e-4 * extent, (name, pos)
        assert nrm <= 1e-4, (name, nrm)
        if rule["has_uv"][real].any():
            assert rule["uv"][1][real].max() <= 1e-4 * np.abs(rule["uv"][0][real]).max(), name


def test_the_rule_agrees_with_itself_and_every_mutation_leaves_the_bound(solved):
    seen = {}
    for name, (data, rays, hits, rule) in solved.items():
        ratios, exact = S.compare(rule, S.as_records(rule))
        assert exact.all() and all(r.max() < 1.0 for r in ratios.values()), name       # the rule's values, rounded to float32, lie inside its own bound
        print(S.report(name, rule, ratios, exact))
    for mutation in S.MUTATIONS:
        name = MUTATION_CASES[mutation]
        data, rays, hits, rule = solved[name]
        wrong = S.as_records(S.surfaces(data, rays, hits, mutate=mutation))
        ratios, exact = S.compare(rule, wrong)
        outside = ~exact | ~(np.maximum.reduce([ratios[k] for k in ("position", "geometric", "shading", "uv")]) < 1.0)
        seen[mutation] = int(outside.sum())
        print("%-28s on %-28s: %d hits outside the bound" % (mutation, name, seen[mutation]))
        assert seen[mutation] >= 1, mutation
    assert seen == MUTATION_MISSES


def test_few_hits_are_undecided(solved):
    for name, (data, rays, hits, rule) in solved.items():
        real = rule["kind"] == 2
        share = float(rule["undecided"][real].mean())
        assert share <= 0.01, (name, share)


def test_misses_and_out_of_range_hits(solved):
    data, rays, hits, rule = solved["sample lds_cache=1"]
    edited = hits.copy(); ei = edited.view(np.int32)
    real = np.nonzero(rule["kind"] == 2)[0]
    ei[real[0], 3] = len(S.raytraced_instances(data))                                   # instance = instanceCount
    k = int(ei[real[1], 3]); mesh = data.meshes[data.instances[S.raytraced_instances(data)[k]].mesh]
    ei[real[1], 4] = len(mesh.indices) // 3                                             # primitive = triCount
    r2 = S.surfaces(data, rays, edited)
    assert r2["kind"][real[0]] == 1 and r2["kind"][real[1]] == 1 and (r2["kind"][real[2:]] == 2).all()
    rec = S.as_records(r2); ri = rec.view(np.uint32)
    miss = np.nonzero(rule["kind"] == 0)[0]
    for row, flags in ((miss[0], 0), (real[0], S.BAD_HIT)):
        assert ri[row, 3] == flags and ri[row, 7] == 0xFFFFFFFF and ri[row, 11] == 0xFFFFFFFF and np.isposinf(rec[row, 14]) and ri[row, 15] == 0
        assert not rec[row, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13]].any()
