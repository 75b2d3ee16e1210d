"""tests/light_rule.py pinned on the CPU: hand-worked values, the oracle's light loop held to the rule pixel by pixel in every scene case of
tests/light_cases.py, and the named wrong variants of the rule, each of which must put the oracle outside the bound somewhere.

The oracle's own G-buffer (shadingPosition, shadingNormal, shadingSpecular, instanceId) goes through the rule and is compared with its directLight.  The bound is
the rule's, the undecided share of a case is capped at 0.5 % of its shaded pixels."""
import numpy as np
import pytest

import light_cases as LC
import light_rule as R

UNDECIDED_CAP = 0.005
_frames, _rules = {}, {}


def _oracle_frame(sample_data, oracle_lib, name):
    """The oracle's frame of a case, rendered once: (scene, view description, frameCount, images)."""
    if name not in _frames:
        from oracle import oracle_py
        d, view, frames = LC.make_case(sample_data, name)
        o = oracle_py.OracleScene(d)
        try:
            for f in range(frames):
                ref = o.render(LC.W, LC.H, images=(f == frames - 1), diSamples=view["di_samples"], maxLights=view["max_lights"])
        finally:
            o.close()
        assert ref["pixelJitter"] == (0.0, 0.0)
        _frames[name] = (d, view, frames - 1, ref)
    return _frames[name]


def _rule_on_oracle(sample_data, oracle_lib, name, mutate=None):
    d, view, frame_count, ref = _oracle_frame(sample_data, oracle_lib, name)
    if mutate is None:                               # the rule itself runs once per case
        if name not in _rules:
            _rules[name] = LC.run_rule(d, view, frame_count, ref["shadingPosition"], ref["shadingNormal"], ref["shadingSpecular"], ref["instanceId"])
        return ref, _rules[name]
    out = LC.run_rule(d, view, frame_count, ref["shadingPosition"], ref["shadingNormal"], ref["shadingSpecular"], ref["instanceId"], mutate=mutate)
    return ref, out


# ---- hand-worked values ----------------------------------------------------------------------------------------------------------------------

def _one_pixel(lights, max_lights, byte, material=None, normal=(0.0, 0.0, 1.0), mutate=None):
    """A 1 x 1 frame: identity view, so rayDirection = (0, 0, -1); the point (0, 0, 0) with specular 0.5; a blue-noise table of one byte value; nothing casts shadows."""
    m = dict(lightGroupMaskBits=1, ignoreNormalFactor=0.0, specularExponent=2.0, shadowRayBias=0.0, selfLight=(0.01, 0.02, 0.03))
    m.update(material or {})
    cam = dict(view=np.eye(4), fov=np.pi / 4, near=0.1, far=1000.0, width=1, height=1, jitter=(0.0, 0.0))
    table = np.full((512, 512, 4), byte, dtype=np.uint8)
    clear = lambda o, d, tmin, tmax, a, b: np.ones(len(o), dtype=np.int8)
    v, b, dec, info = R.direct_light(np.zeros((1, 1, 4)), np.array([[normal]]), np.full((1, 1, 3), 0.5), np.zeros((1, 1), dtype=np.int32), [m], lights,
                                     (0.1, 0.1, 0.1), (0.2, 0.2, 0.2), max_lights, 0, 0, table, cam, clear, mutate=mutate)
    assert dec.all() and (b[0, 0, :3] < 1e-3).all() and v[0, 0, 3] == 1.0
    return v[0, 0, :3]


def _light(pos, col, radius=10.0, exponent=2.0, bits=1):
    return dict(position=pos, diffuseColor=col, attenuationRadius=radius, pointRadius=0.0, specularColor=(1.0, 1.0, 1.0), shadowOffset=0.0,
                attenuationExponent=exponent, groupBits=bits)


A_LIGHT = _light((0.0, 3.0, 4.0), (1.0, 0.5, 0.25))         # distance 5, direction (0, 0.6, 0.8): falloff (1 - 5/10)^2 = 0.25, N.L = 0.8
B_LIGHT = _light((0.0, -3.0, 4.0), (0.2, 0.2, 0.2))         # its mirror image
# Light A alone: Lambert 0.8 * 0.25 = 0.2; reflect(-L, N) = (0, -0.6, 0.8), . (0, 0, 1) = 0.8, * falloff = 0.2, ^2 = 0.04, * specular 0.5 = 0.02;
# light = (1, 0.5, 0.25) * 0.2 + (1, 1, 1) * 0.02 = (0.22, 0.12, 0.07).  Light B: 0.2 * 0.2 + 0.02 = 0.06 in every channel.
A_VALUE, B_VALUE = np.array([0.22, 0.12, 0.07]), np.array([0.06, 0.06, 0.06])
# self light (0.01, 0.02, 0.03); eye light: N . -rayDirection = 1, reflect(rayDirection, N) = (0, 0, 1), . -rayDirection = 1, 1^2 = 1: 0.1 * 1 + 0.2 * 0.5 * 1 = 0.2
REST = np.array([0.21, 0.22, 0.23])


def test_one_pixel_under_one_point_light():
    assert np.allclose(_one_pixel([A_LIGHT], 12, 0), A_VALUE + REST, rtol=0, atol=1e-12)
    assert np.allclose(_one_pixel([A_LIGHT], 1, 255), A_VALUE + REST, rtol=0, atol=1e-12)        # one candidate: probability 1 whatever the byte
    assert np.allclose(_one_pixel([A_LIGHT], 12, 0, material=dict(lightGroupMaskBits=0)), REST, rtol=0, atol=1e-12)       # a mask of 0: nothing from the loop
    assert np.allclose(_one_pixel([A_LIGHT], 12, 0, material=dict(lightGroupMaskBits=2)), REST, rtol=0, atol=1e-12)       # disjoint bits
    assert np.allclose(_one_pixel([A_LIGHT], 0, 0), REST, rtol=0, atol=1e-12)                                            # maxLights 0: no draw
    # beyond its radius a light gives nothing -- unless its exponent is 0: pow(0, 0) = 1, falloff 1: Lambert 0.8, specular 0.5 * 0.8^2 = 0.32
    assert np.allclose(_one_pixel([_light((0.0, 3.0, 4.0), (1.0, 0.5, 0.25), radius=4.0, exponent=1.0)], 12, 0), REST, rtol=0, atol=1e-12)
    assert np.allclose(_one_pixel([_light((0.0, 3.0, 4.0), (1.0, 0.5, 0.25), radius=4.0, exponent=0.0)], 12, 0), np.array([1.12, 0.72, 0.52]) + REST, rtol=0, atol=1e-12)
    # ignoreNormalFactor 1: Lambert = falloff = 0.25 whatever N.L is: (0.25, 0.125, 0.0625) + 0.02
    assert np.allclose(_one_pixel([A_LIGHT], 12, 0, material=dict(ignoreNormalFactor=1.0)), np.array([0.27, 0.145, 0.0825]) + REST, rtol=0, atol=1e-12)


def test_one_pixel_under_two_lights():
    """Simple intensities: falloff * (N.L + 0.707106) * (r + g + b) = 0.25 * 1.507106 * 1.75 for A and * 0.6 for B: A owns the first 1.75 / 2.35 = 0.745 of the range."""
    both = A_VALUE + B_VALUE + REST
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 2, 0), both, rtol=0, atol=1e-12)           # two draws: both lights, no probability
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 2, 204), both, rtol=0, atol=1e-12)         # B first, then A
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 12, 51), both, rtol=0, atol=1e-12)
    # one draw: byte 51 -> r = 0.2 of the range -> A, weighted by total / A's share = 2.35 / 1.75; byte 204 -> 0.8 -> B, weighted by 2.35 / 0.6
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 1, 51), A_VALUE * (2.35 / 1.75) + REST, rtol=0, atol=1e-9)
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 1, 204), B_VALUE * (2.35 / 0.6) + REST, rtol=0, atol=1e-9)
    # 0.745 of 255 is 189.9: byte 189 still draws A, byte 190 draws B
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 1, 189), A_VALUE * (2.35 / 1.75) + REST, rtol=0, atol=1e-9)
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 1, 190), B_VALUE * (2.35 / 0.6) + REST, rtol=0, atol=1e-9)
    # the wrong variants change these numbers as their names say
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 2, 0, mutate="not_zeroed"), 2 * A_VALUE + REST, rtol=0, atol=1e-12)
    assert np.allclose(_one_pixel([A_LIGHT, B_LIGHT], 2, 0, mutate="invprob_always"), A_VALUE * (2.35 / 1.75) + B_VALUE + REST, rtol=0, atol=1e-9)
    # a light behind the surface at N.L = -0.6: the simple intensity does not clamp (bias -0.6 + 0.707 > 0: a candidate), the light itself does: no Lambert term,
    # and no specular term either (the reflected ray points away)
    behind = _light((0.0, 4.0, -3.0), (1.0, 1.0, 1.0))
    assert np.allclose(_one_pixel([behind], 12, 0), REST, rtol=0, atol=1e-12)
    assert np.allclose(_one_pixel([behind], 12, 0, mutate="ndotl_unclamped"), REST - 0.6 * 0.25, rtol=0, atol=1e-12)


def test_blue_noise_addressing_and_the_camera():
    table = np.arange(512 * 512 * 4, dtype=np.uint32).reshape(512, 512, 4)
    px, py = np.array([0, 63, 64, 87]), np.array([0, 63, 64, 71])
    for frame, (tx, ty) in ((0, (0, 0)), (7, (7, 0)), (8, (0, 1)), (63, (7, 7)), (64, (0, 0)), (70, (6, 0))):
        v = R.blue_noise(table.astype(np.float64), px, py, frame, 0).v * 255.0
        assert np.array_equal(np.round(v), table[ty * 64 + py % 64, tx * 64 + px % 64, 0])
    # rayDirection: not normalised; z = -1 for the identity view, x and y the pixel centre over the projection's scales
    cam = dict(view=np.eye(4), fov=np.pi / 2, near=0.1, far=1000.0, width=4, height=2, jitter=(0.0, 0.0))
    d = R.ray_direction(cam)
    assert np.allclose(d[..., 2], -1.0) and np.allclose(d[0, :, 0], np.array([-0.75, -0.25, 0.25, 0.75]) * 2.0) and np.allclose(d[:, 0, 1], [0.5, -0.5])
    assert np.allclose(np.linalg.norm(R.ray_direction(cam, normalised=True), axis=-1), 1.0)


def test_shadow_brute_force_margins():
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    s = R.BruteForceShadows([tri])
    o = np.array([[0.25, 0.25, 1.0], [2.0, 2.0, 1.0], [0.5, 0.5 + 1e-9, 1.0], [0.25, 0.25, 1.0], [0.25, 0.25, 1.0], [0.25, 0.25, 1.0]])
    d = np.tile([0.0, 0.0, -1.0], (6, 1))
    tmin = np.array([0.1, 0.1, 0.1, 0.1, 1.5, 1.0 - 1e-9]); tmax = np.array([5.0, 5.0, 5.0, 0.5, 5.0, 5.0]); z = np.zeros(6)
    # inside; outside; on the edge; ends before the triangle; starts behind it; starts within rounding of it
    assert list(s(o, d, tmin, tmax, z, z)) == [0, 1, -1, 1, 1, -1]


# ---- the oracle, case by case ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LC.CASES)
def test_oracle_direct_light_within_the_rule(sample_data, oracle_lib, name):
    ref, (value, bound, decided, info) = _rule_on_oracle(sample_data, oracle_lib, name)
    lit = info["lit"]
    assert np.array_equal(lit, ref["instanceId"] >= 0) and lit.sum() > 1500
    # the camera restatement against the stored f16 view direction: 2^-11 per component (and the f16 subnormal step)
    rd = R.ray_direction(LC.rule_inputs(_frames[name][0])["camera"])
    assert (np.abs(ref["viewDirection"][..., :3] - rd)[lit] <= 2.0 ** -11 * np.abs(rd[lit]) + 2.0 ** -24).all()
    worst, outside, undecided, mean = LC.compare(ref["directLight"], value, bound, decided)
    n = int(lit.sum())
    shadow, multi, beyond = LC.shares(info)
    print("light_rule oracle %-10s default  ratio=%.6f mean=%.6f undecided=%.3f%% %s shaded=%d in_shadow=%.3f multi=%.3f beyond_four_radii=%.3f"
          % (name, worst, mean, 100.0 * undecided, info["undecided"], n, shadow, multi, beyond))
    assert outside == 0 and worst < 1.0, (outside, worst)
    assert undecided <= UNDECIDED_CAP, undecided
    miss = ~lit
    assert np.array_equal(ref["directLight"][miss], np.tile(np.float32([1, 1, 1, 0]), (int(miss.sum()), 1))) and (ref["directLight"][lit][:, 3] == 1.0).all()
    need = LC.SHARES[name]
    assert shadow >= need[0] and multi >= need[1] and beyond >= need[2], (shadow, multi, beyond, need)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put the oracle outside its bound on more pixels than the case leaves undecided (with the right rule or with the wrong one)."""
    first = LC.MUTATION_CASE[mutation]
    for name in (first,) + tuple(c for c in LC.CASES if c != first):
        ref, (value, bound, decided, info) = _rule_on_oracle(sample_data, oracle_lib, name)
        _, _, und_right, _ = LC.compare(ref["directLight"], value, bound, decided)
        ref, (value, bound, decided, info) = _rule_on_oracle(sample_data, oracle_lib, name, mutate=mutation)
        worst, outside, und_wrong, _ = LC.compare(ref["directLight"], value, bound, decided)
        n = int(info["lit"].sum())
        print("light_rule mutation %-22s case %-10s outside=%d undecided=%d/%d worst ratio=%.3g" % (mutation, name, outside, round(und_wrong * n), round(und_right * n), worst))
        if outside > max(und_right, und_wrong) * n:
            return
    raise AssertionError("no case tells %s from the rule" % mutation)
