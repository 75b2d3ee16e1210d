"""The material-record rule (tests/material_rule.py, rules H1-H10 of DESIGN.md 4) checked on the CPU: hits come from the oracle's traversal (tests/ray_rule.py).

 * tie to the frame: on camera rays of interior pixels of an opaque instance the rule's colour, shading normal and specular agree with the oracle frame's diffuse,
   normal and specular images within half a storage step plus the rule's bound;
 * the bound is not vacuous: at most half a UNORM8 step for colour, specular and shadow alpha, at most 1e-4 for the shading normal, on every case;
 * at most 1 % of the hits are undecided in every case;
 * every wrong variant (`mutate=`) leaves the bound on at least one named case -- the counts measured here are recorded in MUTATION_MISSES.
"""
import numpy as np
import pytest

import material_cases as MC
import material_rule as M
import ray_rule

W, H = 64, 36
HALF_UNORM8, HALF_SNORM16, HALF_F16 = 0.5 / 255.0, 2.0 ** -16, 2.0 ** -11
# mutation -> (case, with the case's lods); hits outside the bound per mutation (the assertion is "at least one", the figures are what was seen)
MUTATION_CASES = {
    "point_level_floor": ("sampler POINT WRAP mipmaps", True),
    "mix_sign_swapped": ("combiner: texel x input, alpha from input", False),
    "mix_on_texel_alpha": ("combiner: texture edge", False),
    "no_detail_scale": ("uvDetailScale 0.5 and 3", False),
    "binormal_sign_dropped": ("sample maps lds_cache=1", False),
    "tangent_not_flipped": ("inside the sphere, no culling", False),
    "shadow_by_solid_multiplier": ("texture edge across 0.3", False),
    "shadow_at_given_lod": ("sampler LINEAR WRAP mipmaps", True),
    "edge_threshold_ge": ("texture edge at 0.3 exactly", False),
    "alpha_after_noise": ("combiner: noise", False),
    "separate_alpha_ignored": ("combiner: texel x input, alpha from input", False),
}
MUTATION_MISSES = {"point_level_floor": 126, "mix_sign_swapped": 462, "mix_on_texel_alpha": 257, "no_detail_scale": 474, "binormal_sign_dropped": 100, "tangent_not_flipped": 205,
                   "shadow_by_solid_multiplier": 400, "shadow_at_given_lod": 367, "edge_threshold_ge": 303, "alpha_after_noise": 484, "separate_alpha_ignored": 175}


@pytest.fixture(scope="module")
def solved(sample_data, oracle_lib):
    """name -> (data, levels, rays, hits, lods, rule without lods, rule with lods): one oracle traversal and two evaluations of the rule per case, shared by the
    tests below and left unchanged."""
    from oracle import oracle_py
    out = {}
    for name, data, seed, options in MC.cases(sample_data):
        o = oracle_py.OracleScene(data)
        try:
            o.render(W, H, images=False)
            rays = ray_rule.random_rays(data, seed, MC.RAYS, floor_instance=3)
            hits = ray_rule.trace(o, rays)
        finally:
            o.close()
        mip = MC.mipmapped(options)
        levels = M.texture_levels(data, mip)
        lods = MC.lods(seed, len(rays), mip)
        out[name] = (data, levels, rays, hits, lods, M.materials(data, levels, rays, hits), M.materials(data, levels, rays, hits, lods))
    return out


def test_the_cases_are_the_ones_named(solved):
    assert list(solved) == MC.NAMES
    for name, (data, levels, rays, hits, lods, r0, r1) in solved.items():
        real = r0["kind"] == 2
        assert real.sum() > MC.RAYS // 20, name
        assert np.array_equal(real, hits.view(np.int32)[:, 3] >= 0), name               # the oracle's hits are all in range
        assert np.abs(data.meshes[3].vertices["uv"]).max() <= 16.0 if "uv" in data.meshes[3].vertices.dtype.names else True
        assert all(max(l[0].shape[:2]) <= 64 for l in levels.values()) or name == "no UV layout"
        assert np.isnan(lods).sum() > 5 and np.isposinf(lods).sum() > 5 and np.isneginf(lods).sum() > 5


def test_lod_clamp():
    """H3: NaN and negative values give 0, +inf the last level, a one-level texture 0."""
    lod = np.array([np.nan, -np.inf, -0.5, -0.0, 0.0, 0.25, 2.5, 3.0, 3.5, np.inf], dtype=np.float32)
    assert M.clamp_lod(lod, 4).tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.25, 2.5, 3.0, 3.0, 3.0]
    assert not M.clamp_lod(lod, 1).any() and not np.signbit(M.clamp_lod(lod, 4)).any()


def test_the_rule_agrees_with_the_oracle_frame(sample_data, oracle_lib):
    """Camera rays of pixels well inside one opaque instance, one-level textures, normal and specular maps on."""
    from oracle import oracle_py
    data = MC.small_sample(sample_data)
    o = oracle_py.OracleScene(data)
    try:
        ref = o.render(W, H)
        hit = ref["primaryHit"]
        inst = np.where(hit[..., 3] == 0xFFFFFFFF, -1, (hit[..., 3] >> 24).astype(np.int64))
        pad = np.pad(inst, 3, mode="edge")
        interior = inst >= 0
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                interior &= pad[3 + dy:3 + dy + H, 3 + dx:3 + dx + W] == inst
        ys, xs = np.nonzero(interior)
        assert len(xs) >= 40 and len(set(inst[ys, xs].tolist())) == 2          # the sphere and the floor
        rays = ray_rule.camera_rays(data, W, H, np.stack([xs, ys], axis=1))
        hits = ray_rule.trace(o, rays)
    finally:
        o.close()
    assert np.array_equal(hits.view(np.int32)[:, 3], inst[ys, xs])
    rule = M.materials(data, M.texture_levels(data), rays, hits)
    assert (rule["kind"] == 2).all() and not rule["undecided"].any()
    want = M.NORMAL_MAPPED | M.SPECULAR_MAPPED | M.TEXTURED | M.VALID
    assert ((rule["flags"] & want) == want).all() and (rule["color"][0][:, 3] > 0.999).all()
    for what, image, step, key in (("colour", ref["diffuse"], HALF_UNORM8, "color"), ("shading normal", ref["shadingNormal"], HALF_SNORM16 + HALF_F16, "normal"),
                                   ("specular", ref["shadingSpecular"], HALF_UNORM8 + HALF_F16, "specular")):
        d = np.abs(rule[key][0][:, :3] - image[ys, xs, :3].astype(np.float64))
        print("%s against the oracle's image: max %.3e (allowed %.3e + the rule's bound, at most %.1e)" % (what, d.max(), step, rule[key][1].max()))
        assert (d <= step + rule[key][1][:, :3]).all(), what


def test_the_bound_is_not_vacuous_and_few_hits_are_undecided(solved):
    for name, (data, levels, rays, hits, lods, r0, r1) in solved.items():
        for tag, rule in (("", r0), (" + lods", r1)):
            real = rule["kind"] == 2
            decided = real & ~rule["undecided"]
            b = {k: float(rule[k][1][decided].max()) for k, _ in M.FIELDS}
            share = float(rule["undecided"][real].mean())
            print("%-44s bounds: colour %.2e, normal %.2e, specular %.2e, shadow alpha %.2e; undecided %.4f" % (name + tag, b["color"], b["normal"], b["specular"], b["shadow"], share))
            assert max(b["color"], b["specular"], b["shadow"]) <= HALF_UNORM8, (name, b)
            assert b["normal"] <= 1e-4, (name, b)
            assert share <= 0.01, (name, share)


def test_flags_follow_the_shader_and_the_hit(solved):
    edge, r_edge = solved["texture edge across 0.3"][0], solved["texture edge across 0.3"][5]
    real = r_edge["kind"] == 2
    cut, shadow_cut = (r_edge["flags"][real] & M.CUTOUT) != 0, (r_edge["flags"][real] & M.SHADOW_CUTOUT) != 0
    assert cut.any() and (~cut).any() and (shadow_cut & ~cut).any()                     # the two multipliers differ: some hits are a hole for shadow rays only
    assert (r_edge["color"][0][real, 3][~cut] == 1.0).all() and (r_edge["color"][0][real, 3][cut] <= M.EDGE).all()
    noise = solved["combiner: noise"][5]
    assert ((noise["flags"][noise["kind"] == 2] & M.NOISE_ALPHA) != 0).all()
    r = solved["no UV layout"][5]
    assert not (r["flags"][r["kind"] == 2] & (M.TEXTURED | M.NORMAL_MAPPED | M.SPECULAR_MAPPED)).any() and not r["lod"].any()
    r = solved["inside the sphere, no culling"][5]
    real = r["kind"] == 2
    assert ((r["flags"][real] & (M.BACK_FACE | M.NORMAL_MAPPED)) == (M.BACK_FACE | M.NORMAL_MAPPED)).sum() > 50
    r = solved["sampler LINEAR WRAP mipmaps"][6]
    assert len(np.unique(r["lod"][r["kind"] == 2])) > 50 and r["lod"].max() <= 3.0 and r["lod"].min() >= 0.0
    r = solved["66 instances, three shaders"][5]
    real = r["kind"] == 2
    assert len(np.unique(r["instance"][real])) > 20 and len(np.unique(r["flags"][real] & (M.NORMAL_MAPPED | M.SPECULAR_MAPPED))) == 3


def test_the_rule_agrees_with_itself_and_every_mutation_leaves_the_bound(solved):
    seen = {}
    for name, (data, levels, rays, hits, lods, r0, r1) in solved.items():
        for tag, rule in (("", r0), (" + lods", r1)):
            ratios, exact = M.compare(rule, M.as_records(rule))
            assert exact.all() and all(r.max() < 1.0 for r in ratios.values()), name       # the rule's values, rounded to float32, lie inside its own bound
            print(M.report(name + tag, rule, ratios, exact))
    assert set(MUTATION_CASES) == set(M.MUTATIONS)
    for mutation in M.MUTATIONS:
        name, with_lods = MUTATION_CASES[mutation]
        data, levels, rays, hits, lods, r0, r1 = solved[name]
        rule = r1 if with_lods else r0
        wrong = M.as_records(M.materials(data, levels, rays, hits, lods if with_lods else None, mutate=mutation))
        ratios, exact = M.compare(rule, wrong)
        outside = ~exact | ~(np.maximum.reduce([ratios[k] for k, _ in M.FIELDS]) < 1.0)
        seen[mutation] = int(outside.sum())
        print("%-28s on %-44s: %d hits outside the bound" % (mutation, name, seen[mutation]))
        assert seen[mutation] >= 1, mutation
    assert seen == MUTATION_MISSES


def test_misses_and_out_of_range_hits(solved):
    data, levels, rays, hits, lods, rule, _ = solved["sample maps lds_cache=1"]
    edited = hits.copy(); ei = edited.view(np.int32)
    real = np.nonzero(rule["kind"] == 2)[0]
    rt = M.S.raytraced_instances(data)
    ei[real[0], 3] = len(rt)                                                            # instance = instanceCount
    k = int(ei[real[1], 3]); mesh = data.meshes[data.instances[rt[k]].mesh]
    ei[real[1], 4] = len(mesh.indices) // 3                                             # primitive = triCount
    r2 = M.materials(data, levels, rays, edited, lods)
    assert r2["kind"][real[0]] == 1 and r2["kind"][real[1]] == 1 and (r2["kind"][real[2:]] == 2).all()
    rec = M.as_records(r2); ri = rec.view(np.uint32)
    miss = np.nonzero(rule["kind"] == 0)[0]
    for row, flags in ((miss[0], 0), (real[0], M.BAD_HIT), (real[1], M.BAD_HIT)):
        assert ri[row, 7] == flags and ri[row, 13] == 0xFFFFFFFF and ri[row, 14] == 0xFFFFFFFF and ri[row, 15] == 0
        assert not ri[row, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12]].any()
