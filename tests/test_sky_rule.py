"""tests/sky_rule.py pinned on the CPU: closed forms of the rule itself, the oracle's sky held to the rule pixel by pixel in every case of tests/sky_cases.py -- through
the rule of the pass that shows it (primary_rule, gi_rule, mirror_rule) --, and the named wrong variants of the rule, each of which must put the oracle outside the rule
in the case built to catch it.

The bounds are the rules' (DESIGN.md E8); at most 0.5 % of the pixels that see the sky in a pass may be undecided (sky_cases.UNDECIDED_CAP)."""
import math

import numpy as np
import pytest

import light_rule as L
import sky_cases as SC
import sky_rule as S
from light_rule import F

_sessions, _rules = {}, {}


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = SC.make_case(sample_data, name)
        r = SC.oracle_session(case)
        _sessions[name] = (case, r[0] if isinstance(r, tuple) else r)
        _rules[name] = {}
    return _sessions[name]


def _rgb(*rows):
    a = np.asarray(rows, dtype=np.float64)
    return [F(a[:, c]) for c in range(3)]


def _values(fs):
    return np.stack([c.v for c in fs], axis=-1)


# ---- closed forms: ModRGBWithHSL (E5) --------------------------------------------------------------------------------------------------------------------

def test_modifier_of_zero_is_the_identity_within_its_bound():
    """RGBtoHSL and back with nothing added returns the colour: one colour from each of the four branches of the two orderings, a primary, a colour past 1."""
    colours = [(0.8, 0.4, 0.2), (0.8, 0.2, 0.4), (0.4, 0.8, 0.2), (0.2, 0.4, 0.8), (0.2, 0.8, 0.4), (0.4, 0.2, 0.8), (1.0, 0.0, 0.0), (0.25, 0.25, 0.75)]
    out, und, part = S.mod_rgb_with_hsl(_rgb(*colours), (0.0, 0.0, 0.0))
    v = _values(out)
    bound = np.stack([c.e for c in out], axis=-1)
    assert not und.any() and (np.abs(v - np.asarray(colours)) <= bound + 1e-15).all() and bound.max() < 2e-6 and part.max() < 1e-6
    # the result is saturated, the colour need not be: (1.1, 0.5, 0.2) comes back as (1, 0.5, 0.2)
    out, _, _ = S.mod_rgb_with_hsl(_rgb((1.1, 0.5, 0.2)), (0.0, 0.0, 0.0))
    assert np.allclose(_values(out)[0], [1.0, 0.5, 0.2], rtol=0, atol=1e-9)                  # (the EPS of (C:22, 37) is in the value: 1e-10)


def test_primaries_and_a_hand_computed_texel():
    """(0.8, 0.4, 0.2): max 0.8, min 0.2, c = 0.6, h = (0.4 - 0.2) / 3.6 = 1 / 18, l = 0.5, s = 0.6 / (1 - 0) = 0.6.  Half a turn of the hue: H = 10 / 18;
    HUEtoRGB = saturate(|10/3 - 3| - 1, 2 - |10/3 - 2|, 2 - |10/3 - 4|) = (0, 2/3, 1); the result (rgb - 0.5) x 0.6 + 0.5 = (0.2, 0.6, 0.8)."""
    out, und, _ = S.mod_rgb_with_hsl(_rgb((0.8, 0.4, 0.2)), (0.5, 0.0, 0.0))
    assert not und.any() and np.allclose(_values(out)[0], [0.2, 0.6, 0.8], rtol=0, atol=1e-9)
    # a third of a turn takes red to green and green to blue; lightness + 0.25 on pure red: c = (1 - |1.5 - 1|) x 1 = 0.5: (1, 0.5, 0.5); saturation - 1 leaves its grey 0.5
    third = float(np.float32(1.0 / 3.0))
    out, _, _ = S.mod_rgb_with_hsl(_rgb((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), (third, 0.0, 0.0))
    assert np.allclose(_values(out), [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], rtol=0, atol=1e-6)
    out, _, _ = S.mod_rgb_with_hsl(_rgb((1.0, 0.0, 0.0)), (0.0, 0.0, 0.25))
    assert np.allclose(_values(out)[0], [1.0, 0.5, 0.5], rtol=0, atol=1e-9)
    out, _, _ = S.mod_rgb_with_hsl(_rgb((1.0, 0.0, 0.0)), (0.0, -1.0, 0.0))
    assert np.allclose(_values(out)[0], [0.5, 0.5, 0.5], rtol=0, atol=1e-9)
    # the wrong variant that adds the saturation modifier to the lightness
    out, _, _ = S.mod_rgb_with_hsl(_rgb((1.0, 0.0, 0.0)), (0.0, 0.0, 0.25), mutate="saturation_on_lightness")
    assert np.allclose(_values(out)[0], [1.0, 0.0, 0.0], rtol=0, atol=1e-9)                # s = 1.25: c = 1.25, saturated back to red


def test_the_hue_is_not_wrapped():
    """(C:12) red has hue 0; a modifier of -0.1 gives H = -0.1, where the three ramps are (2.6, -0.6, -2.6) -> (1, 0, 0): still red.  A wrapped hue, 0.9, is (1, 0, 0.6)."""
    out, und, _ = S.mod_rgb_with_hsl(_rgb((1.0, 0.0, 0.0)), (-0.1, 0.0, 0.0))
    assert np.allclose(_values(out)[0], [1.0, 0.0, 0.0], rtol=0, atol=1e-6)
    out, _, _ = S.mod_rgb_with_hsl(_rgb((1.0, 0.0, 0.0)), (-0.1, 0.0, 0.0), mutate="hue_wrapped")
    assert np.allclose(_values(out)[0], [1.0, 0.0, 0.6], rtol=0, atol=1e-6)
    # past 1 as well: blue, h = 2 / 3, + 0.5: H = 7 / 6 -> (|7 - 3| - 1, 2 - |7 - 2|, 2 - |7 - 4|) = (3, -3, -1) -> (1, 0, 0), not the yellow of H = 1 / 6
    out, _, _ = S.mod_rgb_with_hsl(_rgb((0.0, 0.0, 1.0)), (0.5, 0.0, 0.0))
    assert np.allclose(_values(out)[0], [1.0, 0.0, 0.0], rtol=0, atol=1e-6)


def test_the_one_discontinuity_and_the_three_continuous_boundaries():
    """g = b under a red maximum: the hue is 0 on one side and 1 on the other.  With a hue modifier the two sides differ (undecided where the margin is within the
    errors); with none they agree.  Across r = max(g, b) and across g = b under another maximum the value is continuous: no decision anywhere."""
    eps = 1e-7
    for mod, jumps in (((0.1, 0.0, 0.0), True), ((0.0, 0.2, 0.1), False)):
        a, _, _ = S.mod_rgb_with_hsl(_rgb((0.8, 0.3 + eps, 0.3)), mod)
        b, _, _ = S.mod_rgb_with_hsl(_rgb((0.8, 0.3, 0.3 + eps)), mod)
        gap = np.abs(_values(a) - _values(b)).max()
        assert (gap > 0.1) == jumps and (jumps or gap < 1e-5), (mod, gap)
    near = [F(np.array([0.8]), 1e-7), F(np.array([0.3 + 1e-8]), 1e-7), F(np.array([0.3]), 1e-7)]
    assert S.mod_rgb_with_hsl(near, (0.1, 0.0, 0.0))[1].all() and not S.mod_rgb_with_hsl(near, (0.0, 0.2, 0.1))[1].any()
    grey = [F(np.array([0.5]), 1e-7)] * 3
    assert S.mod_rgb_with_hsl(grey, (0.1, 0.0, 0.0))[1].all()
    far = [F(np.array([0.8]), 1e-7), F(np.array([0.4]), 1e-7), F(np.array([0.3]), 1e-7)]
    assert not S.mod_rgb_with_hsl(far, (0.1, 0.0, 0.0))[1].any()
    for lo, hi in (((0.5 - eps, 0.5, 0.2), (0.5 + eps, 0.5, 0.2)), ((0.5 - eps, 0.2, 0.5), (0.5 + eps, 0.2, 0.5)), ((0.2, 0.6, 0.6 - eps), (0.2, 0.6, 0.6 + eps)),
                   ((0.6, 0.8, 0.2 - 0.0), (0.6 + eps, 0.8, 0.2))):
        a, ua, _ = S.mod_rgb_with_hsl(_rgb(lo), (0.3, 0.2, -0.1)); b, ub, _ = S.mod_rgb_with_hsl(_rgb(hi), (0.3, 0.2, -0.1))
        assert np.abs(_values(a) - _values(b)).max() < 1e-5 and not ua.any() and not ub.any(), (lo, hi)


def test_a_near_grey_is_ill_conditioned_only_under_a_saturation_modifier():
    """c = 2e-6: the hue (g - b) / (6 c) moves by a sixth of a turn with a float32 rounding of a channel.  It reaches the result through (1 - |2 L - 1|) S: s = c / ... is
    4e-6 itself, so without a saturation modifier the hue-conditioning bound stays far below half an f16 step; with one it is as wide as the colour."""
    near_grey = _rgb((0.5 + 2e-6, 0.5 + 1e-6, 0.5))
    _, _, part = S.mod_rgb_with_hsl(near_grey, (0.2, 0.0, 0.0))
    assert part[0] < 1e-5 < S.F16_STEP(0.5)
    _, _, part = S.mod_rgb_with_hsl(near_grey, (0.2, 0.5, 0.0))
    assert part[0] > 0.01 > S.F16_STEP(0.5)
    sky = dict(texels=np.zeros((1, 1, 4), dtype=np.uint8), multiplier=(1.0, 1.0, 1.0), hsl=(0.2, 0.5, 0.0), yawOffset=0.0)
    tex = near_grey + [F(np.ones(1))]
    assert not np.isfinite(S.finish(sky, tex)[0].e).any() and np.isfinite(S.finish(dict(sky, hsl=(0.2, 0.0, 0.0)), tex)[0].e).all()


# ---- closed forms: the colour of a sample (E4, E6) -------------------------------------------------------------------------------------------------------

def test_the_block_is_off_for_zero_and_for_negative_zero():
    """`any(skyHSLModifier)` (S:60) tests != 0: -0.0 is zero.  With the block off the colour is texel x multiplier, not saturated; alpha is the texel's either way."""
    tex = [F(np.array([0.2])), F(np.array([0.4])), F(np.array([0.9])), F(np.array([0.625]))]
    for mod in ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0)):
        out = S.finish(dict(multiplier=(0.5, 0.75, 1.25), hsl=mod), tex)
        assert np.allclose([c.v[0] for c in out], [0.1, 0.3, 1.125, 0.625], rtol=0, atol=1e-12) and max(float(c.e[0]) for c in out) < 2e-7
    on = S.finish(dict(multiplier=(0.5, 0.75, 1.25), hsl=(0.0, 0.0, 1e-6)), tex)
    assert on[2].v[0] <= 1.0 and on[3].v[0] == 0.625
    assert S.finish(dict(multiplier=(0.5, 0.75, 1.25), hsl=(0.0, 0.0, 0.0)), tex, mutate="hsl_when_zero")[2].v[0] <= 1.0
    assert S.finish(dict(multiplier=(0.5, 0.75, 1.25), hsl=(0.0, 0.0, 0.1)), tex, mutate="alpha_modified")[3].v[0] == 0.625 * 1.25


def test_sky_over_background():
    """lerp(bg, sky, a): a = 0.25 of (0.2, 0.4, 0.8, .) over (0.6, 0.6, 0.6) is (0.5, 0.55, 0.65).  At a = 1 it is the sky itself, and its bound holds one rounding more
    than the lerp's: the side that skips the lerp and the side that evaluates it both lie inside."""
    bg = [F(np.array([0.6]))] * 3
    sky = lambda a: [F(np.array([0.2])), F(np.array([0.4])), F(np.array([0.8])), F(np.array([a]))]
    out = S.over_background(bg, sky(0.25))
    assert np.allclose([c.v[0] for c in out], [0.5, 0.55, 0.65], rtol=0, atol=1e-12)
    out = S.over_background(bg, sky(1.0))
    lerp32 = [np.float32(np.float32(0.6) + np.float32(1.0) * (np.float32(x) - np.float32(0.6))) for x in (0.2, 0.4, 0.8)]
    for c, x, y in zip(out, (0.2, 0.4, 0.8), lerp32):
        assert abs(c.v[0] - x) < 1e-15 and abs(float(np.float32(x)) - c.v[0]) <= c.e[0] and abs(float(y) - c.v[0]) <= c.e[0] and c.e[0] < 4e-7
    assert [c.v[0] for c in S.over_background(bg, sky(0.25), mutate="sky_alpha_ignored")] == [0.2, 0.4, 0.8]
    assert [c.v[0] for c in S.over_background(bg, sky(0.75), mutate="shortcut_below_one")] == [0.2, 0.4, 0.8]


# ---- closed forms: the UV of a direction (E1) and of a pixel (E2) ----------------------------------------------------------------------------------------

def _dirs(*rows):
    a = np.asarray(rows, dtype=np.float64)
    return [F(a[:, c], 1e-7) for c in range(3)]


def test_envmap_uv_values_seam_offsets_and_pole():
    """-z is u = 1 / 2, +x is 3 / 4, +z is the seam (0 on one side, 1 on the other: continuous mod 1), level is v = 1 / 2, straight up v = 1 / 4.  A negative offset
    gives a negative u and one past 2 pi wraps; each differs from the offset-free u by offset / 2 pi mod 1, and is the same texel under WRAP.  Straight up or down
    there is no yaw: du is infinite, dv finite."""
    u, v, du, dv = S.fake_envmap_uv(_dirs((0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, -1.0)))
    assert np.allclose(u, [0.5, 0.75, 0.5], atol=1e-12) and np.allclose(v, [0.5, 0.5, 0.375], atol=1e-12) and (du < 1e-6).all() and (dv < 1e-6).all()
    eps = 1e-6
    u, _, _, _ = S.fake_envmap_uv(_dirs((-eps, 0.0, 1.0), (eps, 0.0, 1.0)))
    assert u[0] < 1e-6 and u[1] > 1.0 - 1e-6 and abs((u[0] - u[1]) % 1.0 - 2e-6 / (2.0 * math.pi)) < 1e-9
    d = _dirs((0.3, 0.2, -0.9), (-0.7, -0.1, 0.2), (0.1, 0.5, 0.4), (-0.1, 0.3, 1.0))              # the last one a little past the seam: atan2 + pi = 0.0997
    u0 = S.fake_envmap_uv(d)[0]
    for off in SC.YAW_OFFSETS[1:]:
        u, v, du, _ = S.fake_envmap_uv(d, off)
        turn = float(np.float32(off)) / (2.0 * math.pi)
        assert np.allclose((u - u0 - turn + 0.5) % 1.0, 0.5, atol=1e-9) and (du < 2e-6).all()
        assert (u < 0.0).any() == (off < 0.0) and (u <= 1.0).all()
    sky = dict(texels=SC.texture(3, 16, 8, "rgb"))
    a = S.sample(sky, np.array([-0.3, 0.2]), np.array([0.4, 1.7]), 1e-7, 1e-7); b = S.sample(sky, np.array([0.7, 1.2]), np.array([0.4, 0.7]), 1e-7, 1e-7)
    assert all(np.allclose(x.v, y.v, rtol=0, atol=1e-12) for x, y in zip(a, b))
    u, v, du, dv = S.fake_envmap_uv(_dirs((0.0, 1.0, 0.0), (0.0, -1.0, 0.0)))
    assert np.isinf(du).all() and np.isfinite(dv).all() and np.allclose(v, [0.25, 0.75], atol=1e-12)
    assert S.fake_envmap_uv(_dirs((0.0, 1.0, -1.0)), mutate="pitch_sign")[1][0] == 0.625
    assert not np.isfinite(S.sample(sky, u, v, du, dv)[0].e).any()


def test_plane_base_pitch_clamps_aspect_and_seam():
    """(S:27-47) The camera's backward axis b: yaw = fmod(offset + atan2(b.x, -b.z) + pi, 2 pi), baseX = 640 (yaw - pi) / pi; baseY = 4 x pitch in degrees + 600.
    Looking straight up (b = -y) baseY is SKYBOX_HEIGHT = 960 and baseV = 0; straight down it is SCREEN_HEIGHT = 240 and baseV = 3 / 4: the two ends of the clamp
    are the two ends of atan2's range, so the clamp never moves a value (EQUIVALENT) -- a float32 evaluation may pass an end by a rounding, which the bound holds."""
    level = (0.0, 0.0, 1.0)                                                                     # the default camera looks along -z: b = +z, on the seam
    bu, bv, su, sv, by = S.plane_base(level, 4.0 / 3.0, 0.0)
    assert by == 600.0 and bv == 0.375 and (su, sv) == (0.25, 0.25) and min(abs(bu - 0.5), abs(bu + 0.5)) < 1e-12
    assert S.plane_base((0.0, -1.0, 0.0), 4.0 / 3.0, 0.0)[4] == S.SKYBOX_HEIGHT and S.plane_base((0.0, -1.0, 0.0), 4.0 / 3.0, 0.0)[1] == 0.0
    assert S.plane_base((0.0, 1.0, 0.0), 4.0 / 3.0, 0.0)[4] == S.SCREEN_HEIGHT and S.plane_base((0.0, 1.0, 0.0), 4.0 / 3.0, 0.0)[1] == 0.75
    for pitch in np.linspace(-0.5 * math.pi, 0.5 * math.pi, 181):
        b = (math.cos(pitch) * 0.6, -math.sin(pitch), math.cos(pitch) * 0.8)
        assert abs(S.plane_base(b, 1.5, 0.3)[4] - S.plane_base(b, 1.5, 0.3, mutate="base_y_unclamped")[4]) < 1e-9
    assert S.plane_base((0.0, -0.5, 0.5), 4.0 / 3.0, 0.0, mutate="pitch_sign")[4] == 600.0 - 180.0
    # 45 degrees up: 4 x 45 + 600 = 780 -> (960 - 780) / 960
    assert abs(S.plane_base((0.0, -1.0, 1.0), 4.0 / 3.0, 0.0)[1] - 0.1875) < 1e-12
    # the aspect ratio: 16 : 9 shifts baseU by (160 - 120 x 16 / 9) / 1280 and widens the screen's share to 1 / 3; b = +x is a quarter turn past -z: baseU = (3 pi / 2 - pi) 640 / pi / 1280 = 1 / 4
    bu, _, su, _, _ = S.plane_base((1.0, 0.0, 0.0), 16.0 / 9.0, 0.0)
    assert abs(bu - (0.25 + (160.0 - 120.0 * 16.0 / 9.0) / 1280.0)) < 1e-12 and abs(su - 1.0 / 3.0) < 1e-12
    assert abs(S.plane_base((1.0, 0.0, 0.0), 16.0 / 9.0, 0.0, mutate="aspect_ignored")[0] - 0.25) < 1e-12
    # u is continuous mod 1 across the seam, for a pixel as for a direction; the jitter moves the uv by jitter / size x the factor
    cams = [dict(view=SC.view_matrix(SC.EYE, yaw, 0.1), width=88, height=72, jitter=(0.0, 0.0)) for yaw in (-1e-4, 1e-4)]
    px, py = np.array([0.0, 40.0]), np.array([0.0, 30.0])
    (ua, va, dua, _), (ub, vb, _, _) = (S.sky_plane_uv(c, px, py) for c in cams)
    step = ((ub - ua + 0.5) % 1.0) - 0.5
    assert np.allclose(step, -2e-4 / (2.0 * math.pi), atol=1e-6) and abs(ub[0] - ua[0]) > 0.9 and np.allclose(va, vb, atol=1e-9) and (dua < 1e-5).all()
    j = dict(cams[0], jitter=(0.25, -0.5))
    uj, vj, _, _ = S.sky_plane_uv(j, px, py)
    assert np.allclose(uj - ua, 0.25 / 88.0 * 0.25 * (88.0 / 72.0) / (4.0 / 3.0), atol=1e-12) and np.allclose(vj - va, -0.5 / 72.0 * 0.25, atol=1e-12)
    assert np.allclose(S.sky_plane_uv(j, px, py, mutate="jitter_not_in_sky_uv")[0], ua, atol=1e-15)
    # a camera that looks straight up has no yaw
    up = np.eye(4, dtype=np.float32); up[1, 1] = up[2, 2] = 0.0; up[1, 2] = -1.0; up[2, 1] = 1.0               # the backward axis is exactly -y: the camera looks straight up
    assert S.view_direction(up).tolist() == [0.0, -1.0, 0.0] and np.isinf(S.sky_plane_uv(dict(view=up, width=88, height=72), px, py)[2]).all()


def test_the_tiled_copy_is_the_image_under_another_address():
    """dst[((y / 4) (w / 4) + x / 4) 16 + (y % 4) 4 + x % 4] = src[y w + x] (csrc/bc7.hip) read back through sky_tiled_sample's index is the image; with a wrong row
    pitch it is not, except where the image is one tile high."""
    for w, h in ((64, 32), (16, 8), (4, 4), (8, 32)):
        t = SC.texture(w * h, w, h, "rgb")
        y, x = np.mgrid[0:h, 0:w]
        assert np.array_equal(S.tile(t)[S.tiled_index(x, y, w, h)], t)
        assert np.array_equal(S.tile(t)[S.tiled_index(x, y, w, h, wrong_pitch=True)], t) == (h == 4)
    assert S.can_tile(np.zeros((4, 4, 4))) and not S.can_tile(np.zeros((2, 2, 4))) and not S.can_tile(np.zeros((5, 12, 4))) and not S.can_tile(np.zeros((8, 2, 4)))
    # the padded twin of a texture holds the same texels, under a size that cannot be tiled
    t = SC.texture(7, 64, 32, "rgb"); p = SC.padded(t, 67, 35)
    assert np.array_equal(p[:32, :64], t) and np.array_equal(p[32:, :3], t[:3, :3]) and not S.can_tile(p)


# ---- the oracle, case by case ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SC.CASES)
def test_oracle_sky_within_the_rule(sample_data, oracle_lib, name):
    """Gated cases: nothing outside the rule, ratio < 1, undecided pixels within the cap among those that see the sky.  `record-` cases: run and written down."""
    case, sess = _oracle(sample_data, oracle_lib, name)
    SC.hold(case, sess, "oracle", rules=_rules[name])
    if name == "pole":                  # the level floor sends the bounce ray of blue-noise byte 0 straight up: those pixels have no bound
        for f in case["compared"]:
            rule = _rules[name][f][0][1]
            und = ~rule["decided"] & rule["sky"]
            poles = rule["sky"] & ~np.isfinite(rule["bound"]).all(axis=-1)
            print("sky_rule %-22s %-20s frame %d pixels whose ray leaves straight up: %d of %d undecided" % ("oracle", name, f, poles.sum(), und.sum()))
            assert 0 < poles.sum() <= und.sum() <= int(SC.UNDECIDED_CAP * rule["sky"].sum()) and not rule["decided"][poles].any()
    if name in ("bounce", "bounce-padded"):     # the pair that holds the tiled and the plain device sampler to the one rule: the same scene, the same texels
        assert case["tiled"] == (name == "bounce")


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put the oracle outside the rule, in the case built to catch it (sky_cases.MUTATION_CASE), on more pixels than the frame leaves undecided
    (with the right rule or with the wrong one)."""
    name = SC.MUTATION_CASE[mutation]
    case, sess = _oracle(sample_data, oracle_lib, name)
    f = case["compared"][0]
    if f not in _rules[name]:
        _rules[name][f] = [(SC.inputs_of(case, sess, f), SC.run_rule(case, f, sess))]
    right = SC.judge(case, _rules[name][f][0][1], sess, f)
    wrong = SC.judge(case, SC.run_rule(case, f, sess, mutate=mutation), sess, f)
    print("sky_rule mutation %-26s case %-20s bad=%d of %d undecided=%d/%d" % (mutation, name, wrong["bad"], right["sky"], wrong["undecided_all"], right["undecided_all"]))
    assert right["bad"] == 0
    assert wrong["bad"] > max(right["undecided_all"], wrong["undecided_all"]), "the case built for %s, %s, does not tell it from the rule" % (mutation, name)


@pytest.mark.parametrize("mutation", S.EQUIVALENT)
def test_a_variant_that_is_no_wrong_variant_changes_nothing(sample_data, oracle_lib, mutation):
    """`base_y_unclamped`: the clamp of (S:35) spans the whole range of 4 x pitch + 600, so the rule without it is the rule -- on the steepest cameras of the cases, too."""
    for name in ("up", "down"):
        case, sess = _oracle(sample_data, oracle_lib, name)
        f = case["compared"][0]
        assert SC.judge(case, SC.run_rule(case, f, sess, mutate=mutation), sess, f)["bad"] == 0
