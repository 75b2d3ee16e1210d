"""tests/mirror_rule.py pinned on the CPU: hand-worked single pixels, the oracle's reflection passes and refraction pass held to the rule pixel by pixel in every case of
tests/mirror_cases.py through the session scheme described there (maxReflections is an oracle parameter), and the named wrong variants of the rule, each of which
must put the oracle outside the rule somewhere.

The bound is the rule's; at most 0.5 % of the pixels a pass takes may be undecided (mirror_cases.UNDECIDED_CAP)."""
import numpy as np
import pytest

import light_rule as L
import mirror_cases as MC
import mirror_rule as M

_sessions, _rules = {}, {}


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = MC.make_case(sample_data, name)
        _sessions[name] = (case,) + MC.oracle_sessions(case)
        _rules[name] = {}
    return _sessions[name]


# ---- hand-worked single pixels -------------------------------------------------------------------------------------------------------------------

def _material(**over):
    m = dict(lightGroupMaskBits=1, ignoreNormalFactor=0.0, specularExponent=1.0, shadowRayBias=0.0, selfLight=(0.0, 0.0, 0.0), solidAlphaMultiplier=1.0,
             reflectionFactor=0.0, reflectionFresnelFactor=1.0, reflectionShineFactor=0.0, refractionFactor=0.0, fogEnabled=0, fogMul=1.0, fogOffset=0.0,
             fogColor=(0.0, 0.0, 0.0), depthBias=0.0, specularColor=(0.0, 0.0, 0.0), diffuseColorMix=(0.8, 0.4, 0.2, 1.0))
    m.update(over)
    return m


def _scene(instances, lights=()):
    tris = [i["triangles"] for i in instances]
    return dict(instances=instances, lights=list(lights), ambientBase=(0.25, 0.25, 0.25), ambientNoGI=(0.25, 0.25, 0.25), sky=[L.F(0.0)] * 3,
                bluenoise=np.zeros((512, 512, 4), dtype=np.uint8), frameCount=0, diSamples=0, viewProj=np.eye(4), eyeDiffuse=(0.0, 0.0, 0.0),
                shadow=L.BruteForceShadows(tris))


# a mirror in the plane y = 0 (instance 0; its own triangle lies out of the ray's way) and one triangle 2 above it, facing down (instance 1)
_MIRROR = dict(material=_material(reflectionFactor=0.5, reflectionFresnelFactor=3.0), triangles=np.array([[[100.0, 0.0, 100.0], [101.0, 0.0, 100.0], [100.0, 0.0, 101.0]]]),
               normals=np.tile([0.0, 1.0, 0.0], (1, 3, 1)), transform=np.eye(4), cull=True)


def _above(**material):
    # (0, 2, -4), (4, 2, 4), (-4, 2, 4): e1 x e2 = (0, -64, 0): it faces down
    return dict(material=_material(**material), triangles=np.array([[[0.0, 2.0, -4.0], [4.0, 2.0, 4.0], [-4.0, 2.0, 4.0]]]), normals=np.tile([0.0, -1.0, 0.0], (1, 3, 1)),
                transform=np.eye(4), cull=True)


def _pixel(x):
    return np.asarray(x, dtype=np.float64).reshape(1, 1, -1)


def test_one_mirror_pixel_over_one_triangle():
    """View (0.75, -1, 0) on the mirror y = 0 at the origin: the mirrored direction is (0.75, 1, 0), not normalised, and meets the triangle at t = 2, (1.5, 2, 0).
    Colour (0.8, 0.4, 0.2) = (204, 102, 51) / 255 exactly; no light, so the surface shows ambient 0.5: rgb = colour / 2.  Nothing mirrors there: the new alpha is 0,
    k = alpha = 0.25 and REFLECTION = (0.1, 0.05, 0.025, 0) on top of what was stored."""
    scene = _scene([_MIRROR, _above()])
    r = M.reflection_pass(scene, _pixel([0.0, 0.0, 0.0, 0.0]), _pixel([0.75, -1.0, 0.0]), _pixel([0.0, 1.0, 0.0]), np.zeros((1, 1), dtype=np.int32), _pixel([0.5, 0.0, 0.25, 0.25]))
    assert r["decided"].all() and r["takes"].all() and r["has_hit"].all() and not r["goes_on"].any()
    assert np.allclose(r["value"][0, 0], [0.6, 0.05, 0.275, 0.0], rtol=0, atol=1e-12) and (r["bound"][0, 0, :3] < 1e-3).all()
    assert np.allclose(r["state_position"][0][0, 0], [1.5, 2.0, 0.0], atol=1e-12) and np.allclose(r["state_direction"][0][0, 0], [0.75, 1.0, 0.0], atol=1e-12)
    assert np.allclose(r["state_normal"][0][0, 0], [0.0, -1.0, 0.0], atol=1e-12) and r["state_id"][0, 0] == 1
    # the triangle mirrors as well (factor 0.25).  View (0.25, -0.5, 0): direction (0.25, 0.5, 0), t = 4 at (1, 2, 0); n . d = -0.5, so
    # Fresnel = 0.25 + 0.75 * 0.5^5 * 3 = 0.3203125 with the factor of the MIRRORING instance, 3, not the triangle's own 100; new alpha = 0.3203125 * 1 * 0.25
    scene = _scene([_MIRROR, _above(reflectionFactor=0.25, reflectionFresnelFactor=100.0)])
    r = M.reflection_pass(scene, _pixel([0.0, 0.0, 0.0, 0.0]), _pixel([0.25, -0.5, 0.0]), _pixel([0.0, 1.0, 0.0]), np.zeros((1, 1), dtype=np.int32), _pixel([0.0, 0.0, 0.0, 0.25]))
    na = 0.3203125 * 0.25; k = 0.25 * (1.0 - na)
    assert np.allclose(r["value"][0, 0], [0.4 * k, 0.2 * k, 0.1 * k, na], rtol=0, atol=1e-9) and r["goes_on"].all()
    assert np.allclose(r["state_position"][0][0, 0], [1.0, 2.0, 0.0], atol=1e-12)
    # the view (0, -0.5, -1) sends the ray through the triangle's corner (0, 2, -4): not decided
    r = M.reflection_pass(scene, _pixel([0.0, 0.0, 0.0, 0.0]), _pixel([0.0, -0.5, -1.0]), _pixel([0.0, 1.0, 0.0]), np.zeros((1, 1), dtype=np.int32), _pixel([0.0, 0.0, 0.0, 0.25]))
    assert not r["decided"].any()
    # seen from its back the triangle is culled: the ray ends on nothing, REFLECTION keeps its colour, alpha 0, no state
    r = M.reflection_pass(scene, _pixel([0.0, 4.0, 0.0, 0.0]), _pixel([0.75, 1.0, 0.0]), _pixel([0.0, 1.0, 0.0]), np.zeros((1, 1), dtype=np.int32), _pixel([0.5, 0.0, 0.25, 0.25]))
    assert r["decided"].all() and not r["has_hit"].any() and np.allclose(r["value"][0, 0], [0.5, 0.0, 0.25, 0.0], atol=1e-12)
    # skipped: no surface, or no weight -- the stored value, bound 0
    for ident, alpha in ((-1, 0.25), (0, 1e-7)):
        r = M.reflection_pass(scene, _pixel([0.0, 0.0, 0.0, 0.0]), _pixel([0.75, -1.0, 0.0]), _pixel([0.0, 1.0, 0.0]), np.full((1, 1), ident, dtype=np.int32), _pixel([0.5, 0.0, 0.25, alpha]))
        assert not r["takes"].any() and np.array_equal(r["value"][0, 0], [0.5, 0.0, 0.25, alpha]) and (r["bound"] == 0).all()


def test_one_glass_pixel_and_one_total_internal_pixel():
    """refract(i, n, eta) with i = (0.6, -0.8, 0), n = (0, 1, 0): cos = -0.8.  eta = 0.5: k = 1 - 0.25 * 0.36 = 0.91; direction 0.5 i - (0.5 * -0.8 + sqrt 0.91) n.
    eta = 1.5: k = 1 - 2.25 * 0.36 = 0.19 still refracts; i = (0.8, -0.6, 0): k = 1 - 2.25 * 0.64 < 0: the zero vector, a ray that meets nothing."""
    i, n = L.vec(np.array([[0.6, -0.8, 0.0]])), L.vec(np.array([[0.0, 1.0, 0.0]]))
    d, total, und = M.hlsl_refract(i, n, np.array([0.5]))
    assert not total.any() and not und.any() and np.allclose([c.v[0] for c in d], [0.3, -0.4 - (-0.4 + np.sqrt(0.91)), 0.0], atol=1e-12)
    d, total, und = M.hlsl_refract(L.vec(np.array([[0.8, -0.6, 0.0]])), n, np.array([1.5]))
    assert total.all() and not und.any() and [c.v[0] for c in d] == [0.0, 0.0, 0.0]
    assert not M.hlsl_refract(L.vec(np.array([[0.8, -0.6, 0.0]])), n, np.array([1.5]), mutate="eta_inverted")[1].any()
    # a glass pixel at (0, 4, 0) looking straight down through a pane (normal up) with eta 1: the ray goes on unbent and meets the triangle of instance 1 from ...
    # above: its back, culled.  So: a floor triangle facing up at y = 2, colour / 2 as above, weighted by the refraction alpha 0.5
    up = dict(material=_material(), triangles=np.array([[[0.0, 2.0, -4.0], [-4.0, 2.0, 4.0], [4.0, 2.0, 4.0]]]), normals=np.tile([0.0, 1.0, 0.0], (1, 3, 1)),
              transform=np.eye(4), cull=True)
    pane = dict(_MIRROR, material=_material(refractionFactor=1.0))
    scene = _scene([pane, up])
    r = M.refraction_pass(scene, _pixel([0.0, 4.0, 0.0, 0.0]), _pixel([0.0, -1.0, 0.0]), _pixel([0.0, 1.0, 0.0]), np.zeros((1, 1), dtype=np.int32), _pixel([0.0, 0.0, 0.0, 0.5]))
    assert r["decided"].all() and not r["total_internal"].any() and np.allclose(r["value"][0, 0], [0.2, 0.1, 0.05, 0.5], rtol=0, atol=1e-12)
    # the same pixel under a factor of 1.5 at grazing incidence: total internal, nothing met, no sky: REFRACTION stays (0, 0, 0, alpha)
    scene = _scene([dict(_MIRROR, material=_material(refractionFactor=1.5)), up])
    r = M.refraction_pass(scene, _pixel([0.0, 4.0, 0.0, 0.0]), _pixel([0.8, -0.6, 0.0]), _pixel([0.0, 1.0, 0.0]), np.zeros((1, 1), dtype=np.int32), _pixel([0.0, 0.0, 0.0, 0.5]))
    assert r["decided"].all() and r["total_internal"].all() and np.array_equal(r["value"][0, 0], [0.0, 0.0, 0.0, 0.5])


# ---- the oracle, case by case --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MC.CASES)
def test_oracle_mirror_and_glass_within_the_rule(sample_data, oracle_lib, name):
    case, sess, rays = _oracle(sample_data, oracle_lib, name)
    MC.hold(case, sess, rays, "oracle", rules=_rules[name])
    if name == "lone-pixel":            # pass 1 has work on a few pixels only, its twin on none
        on = int((_rules[name][(0, 0)]["goes_on"]).sum()); assert 0 < on < 0.01 * int(_rules[name][(0, 0)]["takes"].sum()), on
    if name == "lone-pixel-none":
        assert not _rules[name][(0, 0)]["goes_on"].any() and rays[(2, 0)][0] == rays[(1, 0)][0]
    if name == "facing":                # the chain is at least five deep
        assert _rules[name][(0, 4)]["takes"].sum() > 50
    if name == "sky":                   # mirror rays that miss everything, and ones that pass two translucent surfaces
        info = _rules[name][(0, 0)]["info"]; t = _rules[name][(0, 0)]["takes"]
        assert (info["hits"][t] == 0).mean() > 0.2 and (info["contributing"][t] >= 2).mean() > 0.02
    if name == "frames":                # the shard is reached in frames 1, 4 and 6 and not in frame 3
        on = {f: int(_rules[name][(f, 0)]["goes_on"].sum()) for f in case["compared"]}
        assert on[1] > 0 and on[4] > 0 and on[6] > 0 and on[3] == 0, on


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put the oracle outside the rule, in the case built to catch it (mirror_cases.MUTATION_CASE) and no other, on more pixels than the pass leaves
    undecided (with the right rule or with the wrong one)."""
    name = MC.MUTATION_CASE[mutation][0]
    glass = mutation in ("glass_no_shadows", "eta_inverted", "tir_ignored")
    case, sess, rays = _oracle(sample_data, oracle_lib, name)
    assert glass == case["glass"]
    f = case["compared"][0]
    for k in range(1 if glass else case["passes"]):
        if glass:
            right = MC.judge_glass(MC.run_glass(case, sess, f), sess[(0, f)]["refraction"])
            wrong = MC.judge_glass(MC.run_glass(case, sess, f, mutate=mutation), sess[(0, f)]["refraction"])
        else:
            if not (sess[(k, f)]["reflection"][..., 3] > M.EPSILON).any():
                break
            right = MC.judge_pass(MC.run_pass(case, sess, f, k), sess[(k, f)], sess[(k + 1, f)])
            wrong = MC.judge_pass(MC.run_pass(case, sess, f, k, mutate=mutation), sess[(k, f)], sess[(k + 1, f)])
        print("mirror_rule mutation %-24s case %-10s pass %d bad=%d undecided=%d/%d" % (mutation, name, k, wrong["bad"], wrong["undecided"], right["undecided"]))
        assert right["bad"] == 0
        if wrong["bad"] > max(right["undecided"], wrong["undecided"]):
            return
    raise AssertionError("the case built for %s, %s, does not tell it from the rule" % (mutation, name))
