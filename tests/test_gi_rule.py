"""tests/gi_rule.py pinned on the CPU: hand-worked single pixels, the oracle's IndirectRayGen (`pass_indirect` / `gi_ray_radiance`) held to the rule pixel by pixel in
every case of tests/gi_cases.py, and the named wrong variants of the rule, each of which must put the oracle outside the rule in the case built to catch it.

The bound is the rule's; at most 0.5 % of a frame's surface pixels may be undecided (gi_cases.UNDECIDED_CAP)."""
import numpy as np
import pytest

import gi_cases as GC
import gi_rule as G
import light_rule as L

_sessions, _rules = {}, {}


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = GC.make_case(sample_data, name)
        _sessions[name] = (case, GC.oracle_session(case))
        _rules[name] = {}
    return _sessions[name]


# ---- hand-worked single pixels ----------------------------------------------------------------------------------------------------------------------

def _material(colour=(204, 102, 51), **over):
    m = dict(lightGroupMaskBits=1, ignoreNormalFactor=0.0, specularExponent=1.0, shadowRayBias=0.0, selfLight=(0.0, 0.0, 0.0), solidAlphaMultiplier=1.0, depthBias=0.0,
             specularColor=(0.0, 0.0, 0.0), diffuseColorMix=(colour[0] / 255.0, colour[1] / 255.0, colour[2] / 255.0, 1.0))
    m.update(over)
    return m


def _triangle(y, facing, **material):
    """One large triangle in the plane y, over the origin, seen from above ("up") or from below ("down")."""
    t = [[0.0, y, -4.0], [-4.0, y, 4.0], [4.0, y, 4.0]] if facing == "up" else [[0.0, y, -4.0], [4.0, y, 4.0], [-4.0, y, 4.0]]
    return dict(material=_material(**material), triangles=np.array([t]), normals=np.tile([0.0, 1.0 if facing == "up" else -1.0, 0.0], (1, 3, 1)), transform=np.eye(4), cull=True)


def _table(entries=()):
    """A blue-noise table of zeros but for {(slice, channel): byte} at pixel (0, 0): slice f lies at tile (f % 8, f // 8) of 64 x 64 texels."""
    t = np.zeros((512, 512, 4), dtype=np.uint8)
    for (f, channel), byte in dict(entries).items():
        t[(f // 8) * 64, (f % 8) * 64, channel] = byte
    return t


def _scene(instances, table, frame=0, samples=1, bounces=1, sky=(0.0, 0.0, 0.0)):
    return dict(instances=instances, lights=[], ambientBase=(0.125, 0.125, 0.125), ambientNoGI=(0.25, 0.25, 0.25), sky=[L.F(x) for x in sky], skyAlpha=1.0 if any(sky) else 0.0,
                background=None, bluenoise=table, frameCount=frame, diSamples=0, giSamples=samples, giBounces=bounces, giDiffuseStrength=0.5, giSkyStrength=0.5,
                eye=(0.0, 2.0, 10.0), shadow=L.BruteForceShadows([i["triangles"] for i in instances]))


def _pixel(x):
    return np.asarray(x, dtype=np.float64).reshape(1, 1, -1)


def _run(scene, normal=(0.0, 1.0, 0.0), ident=0, **kw):
    return G.indirect(scene, _pixel([0.0, 0.0, 0.0]), _pixel(normal), np.full((1, 1), ident, dtype=np.int32), **kw)


def _luma(rgb):
    return 0.2126 * rgb[0] + 0.7152 * rgb[1] + 0.0722 * rgb[2]


def test_perpendicular_vector_for_a_normal_along_each_axis():
    """(R:41-48) x is chosen only where |x| is STRICTLY the smallest, y only where |y| < |z|: (1, 0, 0) and (0, 1, 0) take z, (0, 0, 1) takes y; the vector is cross(n, axis).
    Then tangent = bitangent x n, and with bn = (1, 0): r = 1, phi = 0, the direction is the tangent itself, along the surface."""
    for n, want in (((1.0, 0.0, 0.0), (0.0, -1.0, 0.0)), ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0)), ((0.0, 0.0, 1.0), (-1.0, 0.0, 0.0)), ((0.25, 0.5, 0.75), (0.0, 0.75, -0.5)),
                    ((-0.5, 0.25, 0.75), (-0.75, 0.0, -0.5))):
        b, und = G.perpendicular_vector(L.vec(np.array([n])))
        assert [float(c.v[0]) for c in b] == list(want) and not und.any(), (n, [float(c.v[0]) for c in b])
    # between values with an error of their own an axis choice closer than the errors is not decided
    n = [L.F(np.array([0.5]), 1e-6), L.F(np.array([0.5 + 1e-7]), 1e-6), L.F(np.array([0.7]), 1e-6)]
    assert G.perpendicular_vector(n)[1].all()
    one, zero = L.F(np.array([1.0])), L.F(np.array([0.0]))
    d, _ = G.bounce_direction(L.vec(np.array([[0.0, 1.0, 0.0]])), one, zero)
    assert np.allclose([c.v[0] for c in d], [0.0, 0.0, 1.0], atol=1e-15) and d[1].v[0] == 0.0 and d[1].e[0] == 0.0          # tangent = (1, 0, 0) x (0, 1, 0)
    d, _ = G.bounce_direction(L.vec(np.array([[0.0, 1.0, 0.0]])), L.F(np.array([0.25])), L.F(np.array([0.25])))               # r = 1 / 2, phi = pi / 2: the bitangent's side
    assert np.allclose([c.v[0] for c in d], [0.5, np.sqrt(0.75), 0.0], atol=1e-15)
    d, _ = G.bounce_direction(L.vec(np.array([[0.0, 1.0, 0.0]])), L.F(np.array([0.25])), L.F(np.array([0.25])), mutate="tangent_swapped")
    assert np.allclose([c.v[0] for c in d], [0.0, np.sqrt(0.75), 0.5], atol=1e-15)


def test_a_ray_that_misses_everything_and_a_pixel_without_a_surface():
    """A zero blue-noise table sends the ray along the normal.  Over the pixel there is nothing: the radiance is ambientBase + sky * giSkyStrength * 1, alpha 1 sample,
    moments (l, l^2).  Without a surface, or with giSamples = 0: ambientBase + ambientNoGI, alpha 0, moments 0."""
    scene = _scene([_triangle(0.0, "up")], _table(), sky=(0.2, 0.4, 0.6))
    r = _run(scene)
    want = [0.125 + 0.5 * x for x in (0.2, 0.4, 0.6)]
    assert r["decided"].all() and np.allclose(r["value"][0, 0], want + [1.0], rtol=0, atol=1e-12) and (r["bound"][0, 0, :3] < 5e-4).all() and r["bound"][0, 0, 3] == 0.0
    assert np.allclose(r["moments"][0, 0], [_luma(want), _luma(want) ** 2], rtol=0, atol=1e-7) and r["info"]["counts"]["miss"] == 1 and r["info"]["counts"]["sky"] == 1
    for ident, samples in ((-1, 1), (0, 0)):
        r = _run(_scene([_triangle(0.0, "up")], _table(), samples=samples, sky=(0.2, 0.4, 0.6)), ident=ident)
        assert np.allclose(r["value"][0, 0], [0.375, 0.375, 0.375, 0.0], rtol=0, atol=1e-12) and (r["moments"] == 0).all() and (r["moments_bound"] == 0).all() and r["decided"].all()


def test_one_pane_before_a_wall():
    """Straight up from the origin: a pane of alpha 0.4 = 102 / 255 at y = 2, colour (0.8, 0.4, 0.2), and an opaque wall at y = 3, colour (0, 0.6, 0.2), both seen from
    below.  colour = pane * 0.4 + wall * 0.6, nothing remains; no light: radiance = ambientBase + colour * (ambientBase + ambientNoGI) * giDiffuseStrength."""
    pane, wall = _triangle(2.0, "down", solidAlphaMultiplier=0.4), _triangle(3.0, "down", colour=(0, 153, 51))
    r = _run(_scene([_triangle(0.0, "up"), pane, wall], _table()))
    colour = [0.8 * 0.4 + 0.0, 0.4 * 0.4 + 0.6 * 0.6, 0.2 * 0.4 + 0.2 * 0.6]
    want = [0.125 + c * 0.375 * 0.5 for c in colour]
    assert r["decided"].all() and np.allclose(r["value"][0, 0, :3], want, rtol=0, atol=1e-9) and r["info"]["counts"]["two_contributing"] == 1
    # the wall's depth bias of 1.5 sorts it first (3 - 1.5 < 2): it is opaque, the pane contributes nothing
    wall_first = _triangle(3.0, "down", colour=(0, 153, 51), depthBias=1.5)
    r = _run(_scene([_triangle(0.0, "up"), pane, wall_first], _table()))
    assert np.allclose(r["value"][0, 0, :3], [0.125 + c * 0.375 * 0.5 for c in (0.0, 0.6, 0.2)], rtol=0, atol=1e-9) and r["info"]["counts"]["two_contributing"] == 0
    # seen from above the pane and the wall are culled: a miss, and no sky
    r = _run(_scene([_triangle(0.0, "up"), _triangle(2.0, "up"), _triangle(3.0, "up")], _table()))
    assert np.allclose(r["value"][0, 0, :3], [0.125] * 3, rtol=0, atol=1e-12) and r["info"]["counts"]["miss"] == 1


def test_the_two_slices_of_a_two_sample_pixel():
    """giSamples = 2 at frame 5: sample 2 reads slice 5 + 2 * 32 = 69 -> 5, sample 1 slice 5 + 32 = 37.  Slice 5 holds (0, 0) at the pixel: straight up, into the wall;
    slice 37 holds (255, 0): r = 1, phi = 0, the ray leaves along the tangent (0, 0, 1) and meets nothing.  The image holds the mean of the two radiances, alpha 2,
    the moments the mean of l and of l^2 -- not l and l^2 of the mean."""
    assert [G.sample_slice(5, s, 2) for s in (2, 1)] == [69, 37] and [G.sample_slice(5, s, 2, mutate="slice_from_zero") for s in (2, 1)] == [37, 5]
    assert [G.sample_slice(7, s, 4) for s in (4, 3, 2, 1)] == [71, 55, 39, 23] and G.sample_slice(0, 1, 1) == 64 and [G.sample_slice(1, s, 3) for s in (3, 2, 1)] == [64, 43, 22]
    table = _table({(37, 0): 255})
    scene = _scene([_triangle(0.0, "up"), _triangle(3.0, "down", colour=(0, 153, 51))], table, frame=5, samples=2, sky=(0.2, 0.4, 0.6))
    r = _run(scene)
    hit = [0.125 + c * 0.375 * 0.5 for c in (0.0, 0.6, 0.2)]
    miss = [0.125 + 0.5 * x for x in (0.2, 0.4, 0.6)]
    assert r["decided"].all() and np.allclose(r["value"][0, 0], [0.5 * (a + b) for a, b in zip(hit, miss)] + [2.0], rtol=0, atol=1e-9)
    assert np.allclose(r["moments"][0, 0], [0.5 * (_luma(hit) + _luma(miss)), 0.5 * (_luma(hit) ** 2 + _luma(miss) ** 2)], rtol=0, atol=1e-7)
    assert r["info"]["counts"]["hit"] == 1 and r["info"]["counts"]["miss"] == 1
    wrong = _run(scene, mutate="moments_of_mean")
    assert abs(wrong["moments"][0, 0, 1] - r["moments"][0, 0, 1]) > 100 * r["moments_bound"][0, 0, 1]
    # at frame 4 neither slice (4, 36) holds the byte: both samples go up
    r = _run(_scene(scene["instances"], table, frame=4, samples=2, sky=(0.2, 0.4, 0.6)))
    assert np.allclose(r["value"][0, 0, :3], hit, rtol=0, atol=1e-9) and r["info"]["counts"]["hit"] == 2


def test_the_slice_and_the_place_of_the_second_bounce():
    """(B1) The second ray reads the slice half-way to the next sample's: + 32 of 64 with one sample, + 16 with two, + 1 where the samples' slices are adjacent.  (B2) Up
    from the origin into a wall at y = 3 (normal down); with zeros in the table the second ray leaves (0, 3, 0) straight down and meets the floor triangle the pixel
    lies on, whose radiance -- ambientBase + floor * ambient * strength -- stands where ambientBase + ambientNoGI stood.  With (255, 0) in the second slice the second
    ray leaves along the wall and brings back ambientBase alone."""
    assert G.second_slice(64, 1) == 96 and G.second_slice(69, 2) == 85 and G.second_slice(71, 4) == 79 and G.second_slice(65, 64) == 66
    assert G.second_slice(64, 1, mutate="second_on_first_slice") == 64
    inst = [_triangle(0.0, "up"), _triangle(3.0, "down", colour=(0, 153, 51))]
    wall, floor = (0.0, 0.6, 0.2), (0.8, 0.4, 0.2)
    r = _run(_scene(inst, _table(), bounces=2))
    second = [0.125 + c * 0.375 * 0.5 for c in floor]
    assert r["decided"].all() and np.allclose(r["value"][0, 0, :3], [0.125 + c * s * 0.5 for c, s in zip(wall, second)], rtol=0, atol=1e-9)
    assert r["info"]["counts"]["hit"] == 2
    r = _run(_scene(inst, _table({(32, 0): 255}), bounces=2))                      # frame 0, one sample: slice 64 -> 0, second slice 96 -> 32
    assert np.allclose(r["value"][0, 0, :3], [0.125 + c * 0.125 * 0.5 for c in wall], rtol=0, atol=1e-9) and r["info"]["counts"]["miss"] == 1
    one = _run(_scene(inst, _table({(32, 0): 255}), bounces=1))
    assert np.allclose(one["value"][0, 0, :3], [0.125 + c * 0.375 * 0.5 for c in wall], rtol=0, atol=1e-9)


# ---- the oracle, case by case -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GC.CASES)
def test_oracle_gi_bounce_within_the_rule(sample_data, oracle_lib, name):
    case, sess = _oracle(sample_data, oracle_lib, name)
    GC.hold(case, sess, "oracle", rules=_rules[name])


@pytest.mark.parametrize("mutation", G.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put the oracle outside the rule, in the case built to catch it (gi_cases.MUTATION_CASE), on more pixels than the frame leaves undecided
    (with the right rule or with the wrong one)."""
    name = GC.MUTATION_CASE[mutation]
    case, sess = _oracle(sample_data, oracle_lib, name)
    f = case["compared"][0]
    if f not in _rules[name]:
        _rules[name][f] = [({k: sess[f][k] for k in GC.INPUTS}, GC.run_rule(case, f, sess[f]))]
    right = GC.judge(_rules[name][f][0][1], sess[f])
    wrong = GC.judge(GC.run_rule(case, f, sess[f], mutate=mutation), sess[f])
    print("gi_rule mutation %-26s case %-18s bad=%d undecided=%d/%d" % (mutation, name, wrong["bad"], wrong["undecided"], right["undecided"]))
    assert right["bad"] == 0
    assert wrong["bad"] > max(right["undecided"], wrong["undecided"]), "the case built for %s, %s, does not tell it from the rule" % (mutation, name)
