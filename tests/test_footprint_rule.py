"""The camera-ray and footprint rule (tests/footprint_rule.py, rules F1-F8 of DESIGN.md 4) checked on the CPU: hits come from the oracle's traversal (tests/ray_rule.py).

 * a closed form: a camera that faces the floor head-on gives the gradients and the lod by hand;
 * tests/sampler_rule.py's primary_rays are reproduced at jitter 0, render size and screen size apart included;
 * on camera rays whose projection amplifies by at most 16 the bound walked in `F` stays below test_gpu_sampler's DLOD = 2^-12, and the grazing floor keeps at
   least 90 % of its pixels there;
 * at most 1 % of the real hits are undecided in every case, for the random rays and for the camera rays -- the caps tests/test_gpu_footprint_query.py uses;
 * every wrong variant (`mutate=`) leaves the bound on at least one hit of the case built for it -- the counts seen here are recorded in MUTATION_MISSES.
"""
import numpy as np
import pytest

import footprint_cases as FC
import footprint_rule as R
import material_cases as MC
import ray_rule
import sampler_rule as SR

UNDECIDED_CAP = 0.01
# mutation -> (case, which rays): "camera" = the rays themselves are compared, "pixels" = footprints of the case's camera rays, "random" = of its random rays
MUTATION_CASES = {
    "jitter_left_out": ("upscaler, third frame", "camera"),
    "render_size_for_screen": ("resolutionScale 0.5", "camera"),
    "dDdy_sign": ("sample, generated mips", "camera"),
    "direction_normalised": ("floor at a grazing angle", "camera"),
    "dO_ignored": ("sample, generated mips", "random"),
    "object_space_corners": ("floor at a grazing angle", "pixels"),
    "detail_scale_not_applied": ("maps of other sizes, detail scales", "pixels"),
    "diffuse_size_for_normal_map": ("maps of other sizes, detail scales", "pixels"),
    "quirk_repaired": ("texel 1 only, maps on", "pixels"),
    "mean_of_extents": ("floor at a grazing angle", "pixels"),
    "clamp_before_positive_test": (None, "degenerate"),
}

# hits (rays) outside the bound per mutation on its case, as seen here (the assertion is "at least one")
MUTATION_MISSES = {"jitter_left_out": 2304, "render_size_for_screen": 2304, "dDdy_sign": 2304, "direction_normalised": 2304, "dO_ignored": 291, "object_space_corners": 847,
                   "detail_scale_not_applied": 1017, "diffuse_size_for_normal_map": 1017, "quirk_repaired": 889, "mean_of_extents": 843}


@pytest.fixture(scope="module")
def solved(sample_data, oracle_lib):
    """name -> dict(case, textures, cam, camera rule, rays / diffs / hits and their rule for the random rays ("random") and for every pixel's camera ray ("pixels")):
    one oracle traversal per set of rays, shared by the tests below and left unchanged."""
    from oracle import oracle_py
    out = {}
    for case in FC.cases(sample_data):
        data = case["data"]
        cam = FC.camera_of(case)
        crule = R.camera_rays(cam, FC.all_pixels(case))
        crays, cdiffs = R.as_rays(crule)
        rays = ray_rule.random_rays(data, case["seed"], FC.RAYS, floor_instance=3)
        diffs = FC.random_diffs(case["seed"], rays)
        o = oracle_py.OracleScene(data)
        try:
            o.render(case["render"][0], case["render"][1], images=False)
            hits, chits = ray_rule.trace(o, rays), ray_rule.trace(o, crays)
        finally:
            o.close()
        textures = R.texture_table(data, generated=FC.mipmapped(case))
        out[case["name"]] = dict(case=case, textures=textures, cam=cam, camera=crule,
                                 random=(rays, diffs, hits, R.footprints(data, textures, rays, diffs, hits)),
                                 pixels=(crays, cdiffs, chits, R.footprints(data, textures, crays, cdiffs, chits)))
    return out


def test_the_cases_are_the_ones_named(solved):
    assert list(solved) == FC.NAMES
    for name, s in solved.items():
        for which in ("random", "pixels"):
            rays, diffs, hits, rule = s[which]
            real = rule["kind"] == 2
            assert real.sum() > len(rays) // 20, (name, which)
            assert np.array_equal(real, hits.view(np.int32)[:, 3] >= 0), (name, which)
        d = s["random"][1]
        assert (np.abs(d[:, 0:3]).sum(axis=1) > 0).sum() > 1000 and (np.abs(d[:, 0:3]).sum(axis=1) == 0).sum() > 500          # dO != 0 and dO = 0
    sizes = solved["maps of other sizes, detail scales"]["textures"]
    assert sizes[4][:2] == (64, 64) and sizes[1][:2] == (32, 32) and sizes[4][2] == 7 and sizes[1][2] == 6
    assert solved["NPOT textures, LINEAR"]["textures"][1] == (5, 3, 3)


def _head_on(sample_data, height):
    """The floor stood up as a wall in the plane z = 0 (object x -> world x, object z -> world -y, ten times as large) under the identity camera moved to
    (0, 0, height); a 65 x 37 frame, whose middle pixel's centre is the optical axis.  (Not a camera that looks straight down: cameraU = W x (0, 1, 0) is 0 there.)"""
    d = MC.small_sample(sample_data)
    v = np.eye(4, dtype=np.float32); v[3, 2] = -height
    d.view = v
    t = np.zeros((4, 4), dtype=np.float32)
    t[0, 0] = 10.0; t[1, 2] = 10.0; t[2, 1] = -10.0; t[3, 3] = 1.0
    d.instances[3].transform = t; d.instances[3].previous_transform = t
    return d


def test_a_camera_facing_the_floor_gives_the_footprint_by_hand(sample_data):
    """The wall is 25 x 20 world units for one unit of u, v (a quad of 2.5 x 2 scaled by 10).  From 40 away, the middle pixel of a 65 x 37 frame covers
    s = 2 * 40 * tan(fov / 2) / 37 units each way: duvdy = (0, s / 20) and dPdy = (0, -s, 0) (pixel y runs down the picture, towards -y, where v grows), and on
    the 64 x 64 tiles lod = log2(64 s / 20).  Across the picture the frame's own sign is kept: its cameraW is view-space +z, which lies BEHIND a right-handed
    camera, so cameraU = W x (0, 1, 0) points to the picture's left and duvdx = (-s / 25, 0), dPdx = (-s, 0, 0) -- the mirror image of the geometric derivative.
    The lods take lengths and do not see it."""
    h, w_, h_ = 40.0, 65, 37
    d = _head_on(sample_data, h)
    cam = R.camera(d, w_, h_)
    crule = R.camera_rays(cam, [[32, 18]])
    rays, diffs = R.as_rays(crule)
    assert np.allclose(rays[0, 0:3], [0, 0, h], atol=1e-5) and np.allclose(rays[0, 4:7], [0, 0, -1], atol=1e-6)
    hits = np.zeros((1, 8), dtype=np.float32); hits[0, 0:3] = (h, 0.4, 0.1); hits.view(np.int32)[0, 3] = 1; hits.view(np.int32)[0, 4] = 1          # (0, 0, 0) lies in triangle 1
    rule = R.footprints(d, R.texture_table(d, generated=True), rays, diffs, hits)
    s = 2.0 * h * np.tan(0.5 * d.fov) / h_
    assert rule["kind"][0] == 2 and rule["has_uv"][0] and rule["textured"][0] and not rule["undecided"][0]
    assert np.allclose(rule["duv"][0][0], [-s / 25.0, 0.0, 0.0, s / 20.0], rtol=1e-6, atol=1e-9)
    assert np.allclose(rule["dP"][0][0], [-s, 0, 0, 0, -s, 0], rtol=1e-6, atol=1e-7)
    want = np.log2(64.0 * s / 20.0)
    assert 1.0 < want < 2.0
    for k in ("lod", "lod_normal", "lod_specular"):          # three maps of 64 x 64, uvDetailScale 1
        assert abs(rule[k]["lod"][0] - want) < 1e-5 and rule[k]["bound"][0] < R.DLOD and rule[k]["taken"][0]
    assert rule["amplification"][0] == pytest.approx(1.0, abs=1e-6)


def test_the_sampler_rules_primary_rays_are_reproduced_at_jitter_zero(sample_data):
    d = MC.small_sample(sample_data)
    px = np.array([[0, 0], [63, 35], [31, 17], [5, 30], [-3, 40], [70, -2]])
    for screen, render in (((64, 36), (64, 36)), ((128, 72), (64, 36)), ((80, 36), (40, 18))):
        cam = R.camera(d, screen[0], screen[1], render[0], render[1])
        rule = R.camera_rays(cam, px)
        origin, D, dDdx, dDdy = SR.primary_rays(cam["view"], d.fov, d.near, d.far, screen[0], screen[1], px[:, 0], px[:, 1], render[0], render[1])
        for got, want in ((rule["origin"][0], np.broadcast_to(origin, (len(px), 3))), (rule["direction"][0], D), (rule["dDdx"][0], dDdx), (rule["dDdy"][0], dDdy)):
            assert np.allclose(got, want, rtol=1e-11, atol=1e-13)
        # the bound is there and small: a few dozen roundings of the vector's own size; compute_ray_diffs subtracts right * |n|^2 - n * (n . right), two vectors
        # of some 5e7 (cameraW is 500 long) whose difference is a few times smaller, and carries the 16 roundings of cameraU / V / W through it: 2^-14 there
        for k, rel in (("origin", 2.0 ** -20), ("direction", 2.0 ** -19), ("dDdx", 2.0 ** -14), ("dDdy", 2.0 ** -14)):
            v, e = rule[k]
            assert (e > 0).all() or k == "origin"
            assert (e <= rel * np.abs(v).max()).all(), k


def test_the_walked_bound_agrees_with_the_sampler_tests_on_camera_rays(solved):
    """Where test_gpu_sampler's derivation applies -- a camera ray, 1 / |cos| <= 16, a lod the clamp does not decide -- the bound walked in F is below its DLOD."""
    seen = 0
    for name, s in solved.items():
        rule = s["pixels"][3]
        for k in ("lod", "lod_normal", "lod_specular"):
            r = rule[k]
            m = (rule["kind"] == 2) & r["taken"] & ~r["undecided"] & ~r["low"] & ~r["high"] & (rule["amplification"] <= R.AMPLIFICATION)
            assert (r["bound"][m] <= R.DLOD).all(), (name, k, float(r["bound"][m].max()))
            seen += int(m.sum())
    assert seen > 2000
    floor = solved["floor at a grazing angle"]["pixels"][3]
    on_floor = (floor["kind"] == 2) & (floor["instance"] == 1)
    assert on_floor.sum() > 500 and (floor["amplification"][on_floor] <= R.AMPLIFICATION).mean() >= 0.9
    assert floor["amplification"][on_floor].max() > 8.0          # ... and grazing it is


def test_few_hits_are_undecided_and_the_bound_is_not_vacuous(solved):
    for name, s in solved.items():
        for which in ("random", "pixels"):
            rule = s[which][3]
            real = rule["kind"] == 2
            share = float(rule["undecided"][real].mean())
            print("%-36s %-7s real %5d undecided %.4f degenerate %d" % (name, which, real.sum(), share, rule["degenerate"][real].sum()))
            assert share <= UNDECIDED_CAP, (name, which, share)
            ok = real & ~rule["degenerate"]
            for key in ("dP", "duv") if rule["has_uv"][ok].any() else ("dP",):
                v, e = rule[key]
                scale = np.abs(v[ok]).max(axis=1)
                assert np.median(e[ok].max(axis=1)[scale > 0] / scale[scale > 0]) < 1e-4, (name, which, key)


def test_flags_lods_and_the_quirk_follow_the_shader(solved):
    q = solved["texel 1 only, maps on"]["pixels"][3]
    real = q["kind"] == 2
    assert q["has_uv"][real].all() and not q["textured"][real].any()
    assert (np.abs(q["duv"][0][real]).max(axis=1) > 0).all()                                          # the gradients are there ...
    assert q["lod_normal"]["taken"][real].all() and not q["lod_normal"]["lod"][real].any()            # ... and the frame hands zeros to the normal map all the same
    assert not q["lod"]["taken"][real].any()
    n = solved["no UV layout"]["random"][3]
    real = n["kind"] == 2
    assert not n["has_uv"][real].any() and not n["duv"][0].any() and np.abs(n["dP"][0][real]).max() > 0
    o = solved["maps of other sizes, detail scales"]["pixels"][3]
    floor = (o["kind"] == 2) & (o["instance"] == 1) & ~o["lod"]["low"] & ~o["lod"]["high"] & ~o["lod_normal"]["low"] & ~o["lod_normal"]["high"]
    assert floor.sum() > 50
    assert np.allclose(o["lod_normal"]["raw"][floor] - o["lod"]["raw"][floor], np.log2(3.0 * 32.0 / 64.0), atol=1e-9)          # detail scale 3 on half the size
    for name, s in solved.items():
        for which in ("random", "pixels"):
            rule = s[which][3]
            for k in ("lod", "lod_normal", "lod_specular"):
                r = rule[k]
                assert np.isfinite(r["lod"]).all() and (r["lod"] >= 0).all() and (r["lod"] <= r["mips"] - 1).all(), (name, which, k)
    # diffs = None is an array of zeros: gradients 0, lods 0
    rays, _, hits, _ = solved["sample, generated mips"]["random"]
    z = R.footprints(solved["sample, generated mips"]["case"]["data"], solved["sample, generated mips"]["textures"], rays, None, hits)
    assert not z["duv"][0].any() and not z["dP"][0].any() and not z["lod"]["lod"].any() and not z["undecided"].any()


def test_the_point_level_is_a_decision_of_its_own(solved):
    """F7 under a POINT sampler: each fetch takes (int)(lod + 0.5); a lod within its bound of a half-integer leaves the hit undecided, and is counted in the cap
    above.  The POINT cases take several levels, on both sides of more than one half-integer; the LINEAR cases carry no level."""
    level, doubt = R.point_level(np.array([0.0, 0.49, 0.5 - 1e-6, 0.5 + 1e-6, 1.2, 2.5, 6.0, 1.3, 1.3]), np.array([0.0, 1e-5, 1e-5, 1e-5, 1e-5, 0.0, 0.0, np.inf, np.nan]))
    assert level.tolist() == [0, 0, 0, 1, 1, 3, 6, 1, 1] and doubt.tolist() == [False, False, True, True, False, False, False, True, True]
    for name, s in solved.items():
        point = "POINT" in name
        for which in ("random", "pixels"):
            rule = s[which][3]
            real = rule["kind"] == 2
            for k in ("lod", "lod_normal", "lod_specular"):
                r = rule[k]
                assert (r["point"][real & r["taken"]] == point).all() and not r["point"][~(real & r["taken"])].any(), (name, which, k)
                assert not r["level_undecided"][~r["point"]].any()
                assert (rule["undecided"] | ~r["level_undecided"]).all()                      # folded into the hit's undecided flag, hence into the cap
            ok, compared = R.compare_levels(rule, R.as_records(rule))                         # the rule's own record selects the rule's own level
            assert ok.all() and (compared > 100) == point, (name, which, compared)
    g = solved["floor at a grazing angle, POINT"]["pixels"][3]
    floor = (g["kind"] == 2) & (g["instance"] == 1)
    counts = np.bincount(g["lod"]["level"][floor], minlength=4)
    assert (counts[:3] > 20).all(), counts                                                            # levels 0, 1 and 2 at least: two half-integers are crossed
    shifted = dict(g, lod=dict(g["lod"], level=g["lod"]["level"] + 1))                                # a level too high is caught
    assert not R.compare_levels(shifted, R.as_records(g))[0][floor].any()


def _outside(rule, mutated):
    """Hits whose mutated record, taken as a device's answer, leaves the rule's bound."""
    ratios, exact, lods_ok = R.compare(rule, R.as_records(mutated))
    bad = ~exact | ~lods_ok
    for r in ratios.values():
        bad |= ~(r < 1.0)
    return bad & (rule["kind"] == 2) & ~rule["undecided"]


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_the_rule_agrees_with_itself_and_every_mutation_leaves_the_bound(solved, mutation):
    name, which = MUTATION_CASES[mutation]
    if which == "degenerate":
        # two corners of the triangle coincide: the barycentric differentials are 0 x inf.  F7's order of comparisons answers 0; the wrong order hands the NaN on
        nan = [R.F(np.array([np.nan])), R.F(np.array([np.nan]))]
        good, bad = R.lod_of(nan, nan, (64, 64, 7)), R.lod_of(nan, nan, (64, 64, 7), mutation)
        assert good["lod"][0] == 0.0 and not (0.0 <= bad["lod"][0] <= 6.0)
        return
    s = solved[name]
    case = s["case"]
    if which == "camera":
        rays, diffs = R.as_rays(s["camera"])
        ratios, exact = R.compare_rays(s["camera"], rays, diffs)
        assert exact.all() and all((r < 1.0).all() for r in ratios.values())
        mrays, mdiffs = R.as_rays(R.camera_rays(s["cam"], FC.all_pixels(case), mutation))
        ratios, exact = R.compare_rays(s["camera"], mrays, mdiffs)
        missed = int(np.any([~(r < 1.0) for r in ratios.values()], axis=0).sum())
    else:
        rays, diffs, hits, rule = s[which]
        assert not _outside(rule, rule).any()
        missed = int(_outside(rule, R.footprints(case["data"], s["textures"], rays, diffs, hits, mutation)).sum())
    print("%-28s on %-36s (%s): %d outside the bound" % (mutation, name, which, missed))
    assert missed >= 1, mutation


def test_misses_and_out_of_range_hits(solved):
    s = solved["sample, generated mips"]
    rays, diffs, hits, rule = s["random"]
    edited = hits.copy(); ei = edited.view(np.int32)
    real = np.nonzero(rule["kind"] == 2)[0]
    ei[real[0], 3] = 2; ei[real[1], 4] = 0x7FFFFFFF; ei[real[2], 3] = 0x7FFFFFFF          # two ray-traced instances: 2 is just past the end
    r = R.footprints(s["case"]["data"], s["textures"], rays, diffs, edited)
    rec = R.as_records(r); ri = rec.view(np.uint32)
    assert (r["kind"][real[:3]] == 1).all() and (r["kind"][real[3:]] == 2).all()
    for rows, flags in ((np.nonzero(r["kind"] == 0)[0], 0), (real[:3], R.BAD_HIT)):
        assert (ri[rows, 7] == flags).all() and (ri[rows, 11] == 0xFFFFFFFF).all() and (ri[rows, 15] == 0xFFFFFFFF).all()
        assert not ri[rows][:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 13, 14]].any()
