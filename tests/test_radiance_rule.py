"""The rule of the radiance queries (tests/radiance_rule.py, rules W1-W12) on the CPU: one ray worked by hand, the conditions every case of tests/radiance_cases.py
must meet before anything runs on a GPU -- the rule alone leaves at most mirror_cases.UNDECIDED_CAP of a case's rays undecided, under both settings of UNSHADOWED,
and every kind of ray the cases are built for occurs at least 16 times -- and the mutations: each wrong variant of the rule changes the answer on the case named
for it, otherwise the cases would not discriminate.  The candidates of a ray come from the oracle's enumeration, as in tests/test_layers_rule.py."""
import numpy as np
import pytest

import layers_cases as LC
import material_rule as M
import mirror_cases
import radiance_cases as RC
import radiance_rule as R
import sky_rule
from light_rule import F

W, H = RC.W, RC.H
# mutation -> (the case on which it must change the answer, the call flags)
MUTATION_CASES = {"lit_first_layer": ("stack_8", 0), "lit_only_lit_layers": ("unlit_8", 0), "eye_light_added": ("stack_3", 0), "fog_after_colour": ("fog_8", 0),
                  "fog_from_camera_default": ("fog_8", 0), "unlit_without_ambient": ("unlit_8", 0), "colour_unquantised": ("stack_8", 0), "sky_unweighted": ("sky_3", 0),
                  "skipped_layer_scales_rem": ("faint_12", 0), "shadowed_under_unshadowed": ("lights_8", R.FLAG_UNSHADOWED)}
_cache = {}


def scene_of(sample_data, name):
    """-> (data, rays, lods)"""
    data, K = RC.case(sample_data, name)
    rays = RC.rays_of(K, RC.SEEDS[name], name=name, data=data)
    lods = np.random.default_rng(len(rays)).uniform(0.0, 2.0, size=len(rays)).astype(np.float32)
    return data, rays, lods


def rule_of(sample_data, name, flags=0, mutate=None):
    key = (name, flags, mutate)
    if key not in _cache:
        data, rays, lods = scene_of(sample_data, name)
        o, cand = LC.enumerate_candidates(data, rays)
        try:
            _cache[key] = R.radiance(data, M.texture_levels(data), rays, cand, lods, flags, R.sky_of(data, W, H), R.view_proj(data, W, H), oracle_scene=o, mutate=mutate)
        finally:
            o.close()
    return _cache[key]


def test_a_ray_down_through_three_sheets_by_hand(sample_data, oracle_lib):
    """From above through sheets of alpha 0.6, 0.4, 0.2 onto the opaque floor: four layers with a weight, coverage complete, the floor is the lit layer, nothing is
    transparent (every layer is lit, no fog), and radiance = surface x light since nothing of the sky is left."""
    data, K = RC.case(sample_data, "stack_3")
    ray = np.zeros((1, 8), dtype=np.float32); ray[0, 0:3] = (0.0, 5.0, 0.0); ray[0, 4:7] = (0.0, -1.0, 0.0); ray[0, 7] = 1000.0
    o, cand = LC.enumerate_candidates(data, ray)
    try:
        r = R.radiance(data, M.texture_levels(data), ray, cand, None, R.FLAG_UNSHADOWED, R.sky_of(data, W, H), R.view_proj(data, W, H), oracle_scene=o)
    finally:
        o.close()
    assert r["layers"][0] == 4 and r["lit"][0] == 3 and r["flags"][0] == R.VALID | R.COVERED | R.LIT and not r["undecided"][0]
    assert r["transmittance"][0][0] == 0.0 and not r["transparent"][0][0].any()
    assert np.allclose(r["radiance"][0][0], r["surface"][0][0] * r["light"][0][0], rtol=0, atol=1e-12)
    assert (r["light"][0][0] > 0.3).all() and (r["radiance"][1][0] < 1e-3).all() and (r["surface"][0][0] > 0.0).any()
    # the same ray shadowed: the sheets above the floor take the light's share away, ambient stays
    o, cand = LC.enumerate_candidates(data, ray)
    try:
        s = R.radiance(data, M.texture_levels(data), ray, cand, None, 0, R.sky_of(data, W, H), R.view_proj(data, W, H), oracle_scene=o)
    finally:
        o.close()
    assert (s["light"][0][0] <= r["light"][0][0]).all() and np.array_equal(s["surface"][0], r["surface"][0])


@pytest.mark.parametrize("name", RC.NAMES)
def test_every_case_meets_its_conditions(sample_data, oracle_lib, name):
    data, rays, _ = scene_of(sample_data, name)
    assert 200 <= len(rays) <= 400
    for flags in (0, R.FLAG_UNSHADOWED):
        r = rule_of(sample_data, name, flags)
        share = r["undecided"].mean()
        print("%-10s flags %#05x rays %3d undecided %.4f %s" % (name, flags, len(rays), share, r["why"]))
        assert share <= mirror_cases.UNDECIDED_CAP, (name, flags, float(share), r["why"])
    r = rule_of(sample_data, name, 0)
    ok = ~r["undecided"] & r["valid"]
    assert (ok & (r["layers"] >= 2)).sum() >= 16 and (~r["valid"]).sum() >= 8
    assert (ok & (r["layers"] == 0)).sum() >= 16                                             # rays that miss everything
    kinds = {"stack_3": r["layers"] == 3, "stack_8": r["layers"] >= 8, "fog_8": r["fogged"] & (r["layers"] >= 2), "unlit_8": r["unlit_last"],
             "edge_8": r["layers"] >= 2, "lights_8": r["shaded_by_walk"], "caster_8": r["shaded_by_walk"], "nosky_3": r["layers"] == 0,
             "sky_3": (r["layers"] == 0) & (r["radiance"][0].max(axis=1) > 0.0), "mirror_3": r["fogged"] & (r["layers"] >= 2),
             "faint_12": r["layers"] >= 10}
    assert (ok & kinds[name]).sum() >= 16, (name, int((ok & kinds[name]).sum()))
    if name == "sky_3":          # the sky those rays leave into is translucent: its colour is the texel's times its alpha, over nothing
        s = R.sky_of(data, W, H)
        alpha = sky_rule.plane_colour(s, [F(rays[:, 4 + c].astype(np.float64)) for c in range(3)])[3].v
        miss = ok & (r["layers"] == 0)
        assert ((alpha[miss] > 0.05) & (alpha[miss] < 0.95)).sum() >= 16


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_changes_the_answer_on_its_case(sample_data, oracle_lib, mutation):
    name, flags = MUTATION_CASES[mutation]
    right, wrong = rule_of(sample_data, name, flags), rule_of(sample_data, name, flags, mutation)
    d = R.differs(right, wrong)
    print("mutation %-28s on %-9s %4d of %4d rays differ" % (mutation, name, int(d.sum()), len(d)))
    assert d.mean() > 0.0, mutation


def test_the_sky_by_the_normalised_direction_is_the_same_sky(sample_data):
    """R.EQUIVALENT: fake_envmap_uv reads ratios of the direction's components, so normalising the direction first moves the uv by no more than its own bound."""
    assert R.EQUIVALENT == ("sky_by_normalised_direction",)
    data, K = RC.case(sample_data, "sky_3")
    rays = RC.rays_of(K, RC.SEEDS["sky_3"])
    d = rays[np.isfinite(rays).all(axis=1) & (np.abs(rays[:, 4:7]).max(axis=1) > 0), 4:7].astype(np.float64)
    unit = d / np.linalg.norm(d, axis=1, keepdims=True)
    a = sky_rule.fake_envmap_uv([F(d[:, c]) for c in range(3)], 0.7)
    b = sky_rule.fake_envmap_uv([F(unit[:, c]) for c in range(3)], 0.7)
    assert (np.abs(a[0] - b[0]) <= a[2] + b[2] + 1e-12).all() and (np.abs(a[1] - b[1]) <= a[3] + b[3] + 1e-12).all()
