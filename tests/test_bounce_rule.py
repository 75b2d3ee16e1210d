"""tests/bounce_rule.py pinned on the CPU.  No CPU path produces bounce records, so the rule is pinned to the picture instead (R9): for the picture cases the
oracle draws a frame without reflection passes (maxReflections = 0); the rule's core, evaluated at the frame's stored G-buffer, is held to the REFLECTION alpha
the primary resolve leaves (R6) within its RGBA16F step; the rule's two directions on the pixels' camera rays are held to reflect / refract of the stored view
direction and normal as mirror_rule states them, within the stored values' steps; the R2 point of those rays and the oracle's hits is held to shadingPosition in
all three components, on a scene with depth-biased opaque instances among them.  Then the rule itself: every case keeps its shares and its
undecided cap, every named wrong variant leaves the bound of the right rule on its case, and hand-worked records give the numbers one can do on paper.
"""
import numpy as np
import pytest

import bounce_cases as BC
import bounce_rule as R
import light_rule as L
import material_cases as MC
import material_rule as M
import mirror_cases as MRC
import mirror_rule as MR
import ray_rule

_rules = {}
PICTURES = ("floor", "facing", "glass", "translucent", "textured", "depth bias")
W, H = 88, 72


def _case_rule(sample_data, name, mutate=None):
    """The rule on the case's own rays and the oracle's hits of them; the unmutated one once per case."""
    if mutate is None and name in _rules:
        return _rules[name]
    data, seed, options, flags = BC.make_case(sample_data, name)
    rays, lods = BC.rays_and_lods(data, name, seed, options)
    key = ("hits", name)
    if key not in _rules:
        _rules[key] = BC.oracle_hits(data, rays, flags)
    rule = R.bounces(data, M.texture_levels(data, MC.mipmapped(options)), rays, _rules[key], lods, mutate=mutate)
    if mutate is None:
        _rules[name] = rule
    return rule


# ---- against the picture (R9) --------------------------------------------------------------------------------------------------------------------------------------

GRAZING = 64.0          # pixels with 1 / |Ng . d| above this are left out of the position comparison (its bound grows with that factor), under GRAZING_CAP
GRAZING_CAP = 0.05      # ... of the held pixels


def _picture_scene(sample_data, name):
    if name == "depth bias":          # bounce_cases' own: the mirror floor (opaque, unfogged) with depthBias 0.25, the sphere with -0.125
        return BC.make_case(sample_data, name)[0]
    return MRC.make_case(MC.small_sample(sample_data), name)["data_at"](0)


@pytest.mark.parametrize("name", PICTURES)
def test_the_rule_gives_the_oracles_primary_resolve(sample_data, oracle_lib, name):
    from oracle import oracle_py
    import surface_rule
    data = _picture_scene(sample_data, name)
    o = oracle_py.OracleScene(data)
    try:
        ref = o.render(W, H, images=True, diSamples=0, maxLights=12, maxReflections=0)
        pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="xy"), axis=-1).reshape(-1, 2)
        rays = ray_rule.camera_rays(data, W, H, pixels)
        hits = ray_rule.trace(o, rays, ray_rule.CULL_BACK_FACING)
    finally:
        o.close()
    assert ref["pixelJitter"] == (0.0, 0.0)
    tab = R.material_table(data)
    inst = np.asarray(ref["instanceId"])
    lit = inst >= 0
    ids = inst[lit]
    # pixels whose first hit is the shaded one, opaque and unfogged: the instance of the oracle's closest hit is the G-buffer's and its material is solid
    first = hits.view(np.int32)[:, 3].reshape(H, W)
    solid = np.asarray([float(data.instances[i].material.solidAlphaMultiplier) >= 1.0 and not data.instances[i].material.fogEnabled for i in
                        surface_rule.raytraced_instances(data)])
    plain = lit & (first == inst) & solid[np.where(inst >= 0, inst, 0)]
    held = plain[lit]
    # R6: the REFLECTION alpha before any pass, an RGBA16F channel, from view and normal as stored (known to half an f16 step)
    g = R.at_gbuffer(ref["shadingPosition"], ref["viewDirection"], ref["shadingNormal"], inst, tab, half_step=L.F16_HALF_STEP)
    alpha = np.asarray(ref["reflection"], dtype=np.float64)[..., 3][lit]
    fv, fe = g["fresnel"]
    fb = fe[:, 0] + np.maximum(L.F16_HALF_STEP * (np.abs(fv[:, 0]) + fe[:, 0]), L.F16_FLOOR)
    ratio_f = np.abs(alpha - fv[:, 0]) / fb
    # The rule on this test's camera rays and the oracle's hits of them.  The oracle makes its camera ray itself: its origin and direction differ from this ray's
    # by up to CAM_K float32 roundings of their largest component -- a shift of the ray of at most cam = CAM_K U reach at the hit, which moves the hit along the
    # ray by cam tan(angle of incidence) <= cam / |Ng . d|.
    rule = R.bounces(data, M.texture_levels(data), rays, hits)
    surf = surface_rule.surfaces(data, rays, hits)
    flat = plain.reshape(-1) & (rule["kind"] == 2) & ~rule["undecided"]
    o64, d64 = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    dlen = np.linalg.norm(d64, axis=1)
    sp = np.asarray(ref["shadingPosition"], dtype=np.float64)[..., :3].reshape(-1, 3)
    reach = np.abs(o64).max(axis=1) + np.linalg.norm(sp - o64, axis=1)
    cam = L.CAM_K * L.U * reach
    with np.errstate(divide="ignore", invalid="ignore"):
        slant = 1.0 / np.abs((surf["geometric"][0] * d64).sum(axis=1) / dlen)
    steep = flat & (slant <= GRAZING)
    left_out = 1.0 - steep.sum() / max(int(flat.sum()), 1)

    def position_ratio(r):          # R2 in all three components: the stored point against the rule's, the along-ray part included
        pv, pe = r["position"]
        return np.linalg.norm(sp - pv, axis=1) / (np.sqrt(3.0) * pe.max(axis=1) + cam * (1.0 + slant) + 1e-300)
    ratio_p = position_ratio(rule)
    # R4 / R5: the rule's directions from the unquantised normal against reflect / refract of the STORED view direction and normal (mirror_rule's statements at
    # the frame's state), within the stored values' half steps through both functions, the rule's own bound and the camera's roundings of the direction
    at = np.cumsum(lit.reshape(-1)) - 1
    gq = R.at_gbuffer(ref["shadingPosition"], ref["viewDirection"], ref["shadingNormal"], inst, tab, half_step=L.F16_HALF_STEP, normal_step=MR.SNORM16_HALF_STEP)
    ratio_d = {}
    for key in ("reflected", "refracted"):
        v, e = gq[key]
        dev = np.abs(rule[key][0][steep] - v[at[steep]])
        ratio_d[key] = (dev / (e[at[steep]] + rule[key][1][steep] + 4.0 * L.CAM_K * L.U * np.abs(d64[steep]).max(axis=1, keepdims=True))).max(axis=1, initial=0.0)
    total = gq["total"]
    print("bounce_rule oracle %-12s shaded %4d held %4d  fresnel ratio max %.4f  position ratio max %.4f (left out as grazing %.4f)  reflected %.4f refracted %.4f  mirror %.3f  total internal %d" %
          (name, int(lit.sum()), int(held.sum()), ratio_f[held].max(initial=0.0), ratio_p[steep].max(initial=0.0), left_out, ratio_d["reflected"].max(initial=0.0),
           ratio_d["refracted"].max(initial=0.0), g["mirror"].mean(), int(total.sum())))
    if name == "glass":          # every surface of this case is translucent or fogged: no pixel for R2 and R6, but the one case whose refract() returns 0
        assert total.sum() >= 20 and not gq["tir_undecided"][total].all()
        return
    assert held.sum() >= 150 and steep.sum() >= 150 and left_out <= GRAZING_CAP
    assert (ratio_f[held] <= 1.0).all(), float(ratio_f[held].max())
    assert (ratio_p[steep] <= 1.0).all(), float(ratio_p[steep].max())
    assert (ratio_d["reflected"] <= 1.0).all() and (ratio_d["refracted"] <= 1.0).all()
    if name == "depth bias":
        # the held pixels lie on biased instances, and the comparison tells R2 from its neighbours: the sort key alone (no bias added back) and the issue's
        # first reading t + depthBias (the bias added to the walk's t) both leave the bound on the floor's pixels
        bias = tab["depthBias"][rule["instance"][steep]]
        assert (bias != 0.0).all() and (bias > 0.0).sum() >= 150
        key_only = position_ratio(R.bounces(data, M.texture_levels(data), rays, hits, mutate="no_depth_bias"))[steep]
        moved = rule["position"][0] + d64 * tab["depthBias"][np.where(rule["instance"] >= 0, rule["instance"], 0)][:, None]
        added = (np.linalg.norm(sp - moved, axis=1) / (np.sqrt(3.0) * rule["position"][1].max(axis=1) + cam * (1.0 + slant) + 1e-300))[steep]
        print("    depth bias: held pixels %d; outside the bound with the sort key alone %d, with t + depthBias %d" % (int(steep.sum()), int((key_only > 1.0).sum()), int((added > 1.0).sum())))
        assert (key_only > 1.0).mean() >= 0.9 and (added > 1.0).mean() >= 0.9


# ---- the rule itself -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BC.NAMES)
def test_every_case_is_worth_running(sample_data, oracle_lib, name):
    rule = _case_rule(sample_data, name)
    sh = R.shares(rule)
    real = int((rule["kind"] == 2).sum())
    print("bounce_rule case %-22s hits %4d of %4d  mirror %.3f  glass %.3f  total internal %.3f  back %.3f  mapped %.3f  undecided %.4f %s" %
          ((name, real, len(rule["kind"])) + sh + (rule["why"],)))
    assert 1000 <= len(rule["kind"]) <= 2000 and real >= 400 and real < len(rule["kind"]) - 100          # a share of the rays misses
    assert all(a >= b for a, b in zip(sh[:5], BC.SHARES[name])), (sh, BC.SHARES[name])
    assert sh[5] <= BC.UNDECIDED_CAP
    # the records the rule would store pass its own comparison: the float32 rounding of a value is inside its bound
    ratios, exact = R.compare(rule, R.as_records(rule))
    assert exact.all() and all((r <= 0.51).all() for r in ratios.values())


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put the right rule's records outside its bound on more records than either leaves undecided."""
    name = BC.MUTATION_CASE[mutation]
    right = _case_rule(sample_data, name)
    wrong = _case_rule(sample_data, name, mutate=mutation)
    with np.errstate(invalid="ignore"):
        ratios, exact = R.compare(wrong, R.as_records(right))
    out = ~exact
    for r in ratios.values():
        out |= ~(r <= 1.0)
    und = int((wrong["undecided"] | right["undecided"]).sum())
    print("bounce_rule mutation %-24s case %-16s outside=%d undecided=%d" % (mutation, name, int(out.sum()), und))
    assert out.sum() > und


def test_the_expressions_are_mirror_rules(sample_data, oracle_lib):
    """reflect and refract ARE mirror_rule's functions; the Fresnel amount equals its lines (M:19-23) evaluated on a case's own normals and directions."""
    assert R.reflect3 is L.reflect3 and R.hlsl_refract is MR.hlsl_refract
    rule = _case_rule(sample_data, "facing")
    data, seed, options, flags = BC.make_case(sample_data, "facing")
    rays, _ = BC.rays_and_lods(data, "facing", seed, options)
    mat = M.materials(data, M.texture_levels(data), rays, _rules[("hits", "facing")])
    i = np.nonzero(rule["kind"] == 2)[0]
    n = [L.F(mat["normal"][0][i, c], mat["normal"][1][i, c]) for c in range(3)]
    d = [L.F(rays[i, 4 + c].astype(np.float64)) for c in range(3)]
    tab = R.material_table(data)
    rf, ff = tab["reflectionFactor"][rule["instance"][i]], tab["reflectionFresnelFactor"][rule["instance"][i]]
    base = L.add(1.0, L.dot3(n, d))
    fres = L.add(rf, L.mul(L.mul(L.sub(1.0, rf), L.power(MR.clamp(base, MR.EPSILON, 1.0), 5.0)), ff))
    mirror = rf > MR.EPSILON
    assert mirror.sum() > 100
    assert np.array_equal(np.where(mirror, fres.v, 0.0), rule["fresnel"][0][i, 0])


# ---- hand-worked records -----------------------------------------------------------------------------------------------------------------------------------------------

def _hand_scene(sample_data, **floor_material):
    """small_sample without its maps (the floor's normal is (0, 1, 0)); the floor's second triangle at u = 0.25, v = 0.5 is the point (3.75, 0, 5)."""
    from sm64rt_legacy_renderer_amd import rt64
    d = MC.small_sample(sample_data)
    d.shader_flags = rt64.SHADER_RASTER_ENABLED | rt64.SHADER_RAYTRACE_ENABLED
    for k, v in floor_material.items():
        setattr(d.instances[3].material, k, v)
    return d


def _hand_record(d, origin, direction, t):
    rays = np.zeros((1, 8), dtype=np.float32); rays[0, 0:3] = origin; rays[0, 4:7] = direction; rays[0, 7] = np.inf
    hits = np.zeros((1, 8), dtype=np.float32); hits[0, 0:3] = (t, 0.25, 0.5)
    hits.view(np.int32)[0, 3] = 1; hits.view(np.uint32)[0, 4] = 1
    rule = R.bounces(d, M.texture_levels(d), rays, hits)
    assert not rule["undecided"].any()
    return rule


def test_hand_worked_records(sample_data):
    close = lambda a, b: np.allclose(a, b, rtol=0, atol=1e-6)
    # normal incidence with a direction of length 2: N . d = -2, 1 + N . d = -1, floored at 1e-6: fresnel = rf + (1 - rf) 1e-30 ff = rf.  reflect = d - 2 (-2) N =
    # (0, 2, 0), NOT normalised.  refract at eta 0.5: k = 1 - 0.25 (1 - 4) = 1.75; 0.5 d - (0.5 (-2) + sqrt 1.75) N = (0, -1 - 0.3229, 0).  The point: t = 2.5,
    # depthBias 0.25: (3.75, 5, 5) + (0, -2, 0) ((2.5 - 0.25) + 0.25) = (3.75, 0, 5): on the floor, where the frame puts it (the bias orders hits, it moves none).
    d = _hand_scene(sample_data, reflectionFactor=0.25, reflectionFresnelFactor=2.0, refractionFactor=0.5, depthBias=0.25)
    r = _hand_record(d, (3.75, 5.0, 5.0), (0.0, -2.0, 0.0), 2.5)
    assert r["flags"][0] == R.VALID | R.MIRROR | R.GLASS
    assert close(r["fresnel"][0][0], 0.25) and close(r["position"][0][0], (3.75, 0.0, 5.0))
    assert close(r["reflected"][0][0], (0.0, 2.0, 0.0)) and close(r["refracted"][0][0], (0.0, -1.0 - (np.sqrt(1.75) - 1.0), 0.0))
    assert r["tmin"][0] == np.float32(0.1) and r["tmax"][0] == np.float32(100000.0)
    # k exactly negative: eta 1.5 at 60 degrees from the normal, d = (sin 60, -cos 60, 0): k = 1 - 2.25 (1 - 0.25) = -0.6875: the zero direction and the flag;
    # not a mirror: fresnel 0 though 1 + N . d = 0.5
    d = _hand_scene(sample_data, reflectionFactor=0.0, reflectionFresnelFactor=2.0, refractionFactor=1.5)
    r = _hand_record(d, (3.75 - 5.0 * np.sqrt(0.75), 2.5, 5.0), (np.sqrt(0.75), -0.5, 0.0), 5.0)
    assert r["flags"][0] == R.VALID | R.GLASS | R.TOTAL_INTERNAL
    assert close(r["refracted"][0][0], 0.0) and (r["refracted"][1][0] < 1e-30).all() and close(r["fresnel"][0][0], 0.0)
    assert close(r["reflected"][0][0], (np.sqrt(0.75), 0.5, 0.0)) and close(r["position"][0][0], (3.75, 0.0, 5.0))
    # from below: the back face, the normal turned to (0, -1, 0); d = (0, 0.5, 0): 1 + N . d = 0.5, fresnel = 0.5 + 0.5 x 0.5^5 x 1 = 0.515625, reflect (0, -0.5, 0)
    d = _hand_scene(sample_data, reflectionFactor=0.5, reflectionFresnelFactor=1.0)
    r = _hand_record(d, (3.75, -5.0, 5.0), (0.0, 0.5, 0.0), 10.0)
    assert r["flags"][0] == R.VALID | R.BACK_FACE | R.MIRROR
    assert close(r["fresnel"][0][0], 0.515625) and close(r["reflected"][0][0], (0.0, -0.5, 0.0))
    # a miss and two bad hits: R1's records
    for instance, prim, flags in ((-1, 0, 0), (99, 0, R.BAD_HIT), (1, 2, R.BAD_HIT)):
        rays = np.zeros((1, 8), dtype=np.float32); rays[0, 4:7] = (0.0, -1.0, 0.0)
        hits = np.zeros((1, 8), dtype=np.float32); hits.view(np.int32)[0, 3] = instance; hits.view(np.uint32)[0, 4] = prim
        rule = R.bounces(d, M.texture_levels(d), rays, hits)
        rec, refl, refr = R.as_records(rule)
        ri = rec.view(np.uint32)[0]
        assert rule["kind"][0] == (0 if instance < 0 else 1)
        assert ri[3] == flags and ri[4] == 0xFFFFFFFF and ri[5] == 0xFFFFFFFF and not ri[[0, 1, 2, 6, 7]].any()
        assert not refl.view(np.uint32).any() and not refr.view(np.uint32).any()
