"""The sky of one frame as a rule in numpy float64 (rules E1-E8).  TEST INFRASTRUCTURE.

`fake_envmap_uv`, `sky_plane_uv`, `sky_tiled_sample`, `sky_finish`, `mod_rgb_with_hsl` and `sky_over_background_*` (csrc/shade.h), the view-only half of the sky plane's
UV (`P.skyBase`, csrc/rt64_host.cpp), the tiled copy (`tile_texture_kernel`, csrc/bc7.hip) and their C restatement in oracle/oracle_shade.c were written from the same
HLSL by the same hand.  This module states the sky a third time, from its meaning (BgSky.hlsli:14-95, cited as (S:n); Color.hlsli:9-43, cited as (C:n)), in float64,
with the `F` arithmetic of tests/light_rule.py: every value carries a first-order bound on what a float32 evaluation may differ by, and a sample whose colour hangs on
a decision closer than DECISION_K x the error of its two sides, or on a direction without a finite yaw, gets an infinite bound: the rule that asked for it reports the
pixel undecided.  It imports nothing from oracle/ and nothing from the library.

A sky is described by a dict: texels ((H, W, 4) bytes: level 0 of the sky plane's texture), multiplier, hsl (three floats each), yawOffset, and `mutate` (a wrong
variant of this module, or None).  The rule knows ONE sampler -- LINEAR / WRAP at level 0 -- and both device samplers (`tex_sample_level` and `sky_tiled_sample`) are
held to it.
"""
import math

import numpy as np

import light_rule as L
from light_rule import F

DECISION_K = L.DECISION_K
ANGLE_K = 8                                          # upper estimate of the float32 roundings of atan2 and the sum and fmod around it (S:15-16), in units of U x the angle
PLANE_K = 16                                         # upper estimate of the float32 roundings between the normalised view direction and baseUV (S:27-49), in units of U x (1 + |uv|)
SCREEN_UV_K = 4                                      # roundings of a Halton value, p + jitter and the quotient by the size
CAM_K = L.CAM_K                                      # roundings of the inverse view matrix and the normalisation behind viewDirection (S:24)
SCREEN_WIDTH, SCREEN_HEIGHT = 320.0, 240.0           # (S:9-12)
SKYBOX_WIDTH, SKYBOX_HEIGHT = 4.0 * SCREEN_WIDTH, 4.0 * SCREEN_HEIGHT
HSL_EPS = float(np.float32(1e-10))                   # (C:7)
HUE_K = 4                                            # float32 roundings of a channel before RGBtoHCV reads it: the texel's decode, two of the bilinear mix, the multiplier
F16_STEP = lambda v: np.maximum(L.F16_HALF_STEP * np.abs(v), L.F16_FLOOR)        # half a step of an RGBA16F channel at the value
UNORM8_STEP = lambda v: np.full(np.shape(v), 0.5 / 255.0)                        # half a step of an RGBA8 channel

MUTATIONS = ("yaw_offset_ignored", "yaw_offset_on_background", "pitch_sign", "aspect_ignored", "jitter_not_in_sky_uv", "clamp_instead_of_wrap",
             "nearest_instead_of_linear", "tile_row_stride", "multiplier_after_hsl", "hsl_when_zero", "hue_wrapped", "saturation_on_lightness", "alpha_modified",
             "sky_alpha_ignored", "shortcut_below_one")
# (E2) 4 x pitch in degrees + 600 lies in [240, 960] for every pitch in [-90, 90] degrees: the clamp of (S:35) is the identity on the whole range of atan2, and the
# variant without it is no wrong variant.  tests/test_sky_rule.py pins that.
EQUIVALENT = ("base_y_unclamped",)


def described(sky):
    """A sky description (a dict), not the one constant term of the scenes without UV arithmetic."""
    return isinstance(sky, dict)


def _f32(x):
    return float(np.float32(x))


# ---- arithmetic that stays defined beside an infinite bound ------------------------------------------------------------------------------------------------

def _p(x, y):
    """x y with 0 x inf = 0: an exact zero has no error to scale."""
    with np.errstate(invalid="ignore"):
        r = np.asarray(x, dtype=np.float64) * np.asarray(y, dtype=np.float64)
    return np.where((np.asarray(x) == 0.0) | (np.asarray(y) == 0.0), 0.0, r)


def _mul(a, b):
    a, b = L._f(a), L._f(b)
    v = a.v * b.v
    return F(v, _p(np.abs(a.v), b.e) + _p(np.abs(b.v), a.e) + _p(a.e, b.e) + L.U * np.abs(v))


def _div(a, b):
    """a / b of a positive b (1-ulp reciprocal, one product); no finite bound where b's interval reaches zero."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lo = b.v - b.e
        ok = lo > 0.0
        v = a.v / b.v
        e = np.where(ok, a.e / np.where(ok, lo, 1.0) + np.abs(a.v) * b.e / (b.v * np.where(ok, lo, 1.0)), np.inf) + (L.A + L.U) * np.abs(v)
    return F(v, np.where((a.v == 0.0) & (a.e == 0.0), 0.0, e))


def _abs(a):
    return F(np.abs(a.v), a.e)


def _min2(a, b):
    return F(np.minimum(a.v, b.v), np.maximum(a.e, b.e))


# ---- E1: the UV of a direction -----------------------------------------------------------------------------------------------------------------------------

def fake_envmap_uv(d, yaw_offset=0.0, mutate=None):
    """(E1, S:14-18) (fmod(yawOffset + atan2(x, -z) + pi, 2 pi), fmod(atan2(-y, sqrt(x^2 + z^2)) + pi, 2 pi)) / 2 pi.  d: three F.  Returns (u, v, du, dv): the error of a
    float32 evaluation is that of the angles -- the direction's own error seen from the axis, ANGLE_K roundings of the angle and of the offset beside it -- over 2 pi.
    fmod keeps the sign of the sum: a negative yawOffset gives u < 0, a sum past 2 pi wraps; neither is a decision, because under WRAP addressing u, u + 1 and u - 1
    are the same place.  A direction with no horizontal part has no yaw: du is infinite."""
    x, y, z = d
    off = _f32(yaw_offset)
    hx = np.hypot(x.v, z.v); hl = np.sqrt(hx * hx + y.v * y.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        yaw_e = np.where(hx > 0.0, (x.e + z.e) / hx, np.inf)
        pitch_e = np.where(hl > 0.0, (x.e + y.e + z.e) / hl, np.inf)
    yaw = np.fmod(off + np.arctan2(x.v, -z.v) + math.pi, 2.0 * math.pi)
    pitch = np.fmod(np.arctan2(y.v if mutate == "pitch_sign" else -y.v, hx) + math.pi, 2.0 * math.pi)
    k = ANGLE_K * L.U * 2.0 * math.pi
    return yaw / (2.0 * math.pi), pitch / (2.0 * math.pi), (yaw_e + k + ANGLE_K * L.U * abs(off)) / (2.0 * math.pi) + 2.0 * L.U, (pitch_e + k) / (2.0 * math.pi) + 2.0 * L.U


# ---- E2: the UV of a pixel ---------------------------------------------------------------------------------------------------------------------------------

def view_direction(view):
    """(S:24) normalize(mul(viewI, (0, 0, 1, 0)).xyz): the camera's backward axis in the world -- with row vectors, the third row of the inverse view matrix."""
    vi = np.linalg.inv(np.asarray(view, dtype=np.float32).astype(np.float64))
    d = vi[2, :3]
    return d / np.linalg.norm(d)


def plane_base(vd, aspect, yaw_offset, mutate=None):
    """(E2, S:27-47) baseUV and the two factors of the pixel's uv from the view direction (three floats): (baseU, baseV, 0.25 x ratioDivision, 0.25), and baseY before
    the division, for the tests."""
    off = 0.0 if mutate == "yaw_offset_ignored" else _f32(yaw_offset)
    yaw = math.fmod(off + math.atan2(vd[0], -vd[2]) + math.pi, 2.0 * math.pi)                                  # (S:27)
    base_x = SCREEN_WIDTH * 360.0 * (yaw - math.pi) / (90.0 * math.pi * 2.0)                                   # (S:28)
    pitch = math.atan2(vd[1] if mutate == "pitch_sign" else -vd[1], math.hypot(vd[0], vd[2]))                  # (S:31)
    base_y = 360.0 * (pitch * 360.0 / (math.pi * 2.0)) / 90.0 + 5.0 * (SCREEN_HEIGHT / 2.0)                    # (S:32-34)
    if mutate != "base_y_unclamped":
        base_y = min(max(base_y, SCREEN_HEIGHT), SKYBOX_HEIGHT)                                                # (S:35)
    if mutate == "aspect_ignored":
        aspect = 4.0 / 3.0
    base_x = (base_x + SCREEN_WIDTH / 2.0 - (SCREEN_HEIGHT * aspect) / 2.0) / SKYBOX_WIDTH                     # (S:39-43)
    return base_x, (SKYBOX_HEIGHT - base_y) / SKYBOX_HEIGHT, 0.25 * (aspect / (4.0 / 3.0)), 0.25, base_y      # (S:44-49)


def sky_plane_uv(camera, px, py, yaw_offset=0.0, mutate=None):
    """(E2, S:20-52) the sky plane's uv of pixels.  camera: view (4 x 4 float32, as the host sent it), width, height, jitter (x, y).  screenUV = (p + jitter) / size, no
    half pixel (PrimaryRayGen.hlsl:47).  Returns (u, v, du, dv).  A camera that looks straight up or down has no yaw: du is infinite."""
    w, h = float(camera["width"]), float(camera["height"])
    jx, jy = (0.0, 0.0) if mutate == "jitter_not_in_sky_uv" else camera.get("jitter", (0.0, 0.0))
    vd = view_direction(camera["view"])
    bu, bv, su, sv, _ = plane_base(vd, w / h, yaw_offset, mutate)
    hx = math.hypot(vd[0], vd[2])
    e = CAM_K * L.U
    yaw_e = 2.0 * e / hx if hx > 0.0 else np.inf
    pitch_e = 3.0 * e
    sx, sy = (np.asarray(px, dtype=np.float64) + jx) / w, (np.asarray(py, dtype=np.float64) + jy) / h
    u, v = bu + sx * su, bv + sy * sv
    # d baseU / d yaw = 1 / (2 pi); d baseV / d pitch = 4 x (180 / pi) / 960
    du = yaw_e / (2.0 * math.pi) + (ANGLE_K * abs(_f32(yaw_offset)) + PLANE_K * (1.0 + np.abs(u)) + SCREEN_UV_K * su) * L.U
    dv = pitch_e * 4.0 * (180.0 / math.pi) / SKYBOX_HEIGHT + (PLANE_K * (1.0 + np.abs(v)) + SCREEN_UV_K * sv) * L.U
    return u, v, du, dv


# ---- E3: the sample ----------------------------------------------------------------------------------------------------------------------------------------

def tiled_index(x, y, w, h, wrong_pitch=False):
    """The place of texel (x, y) in the copy kept in 4 x 4 tiles, one tile after the other, rows of tiles top to bottom (csrc/bc7.hip)."""
    lw = int(w).bit_length() - 1
    pitch = (lw - 1) if wrong_pitch else (lw - 2)
    return ((((y >> 2) << pitch) + (x >> 2)) * 16 + ((y & 3) << 2) + (x & 3)) % (w * h)


def tile(texels):
    """The tiled copy of an (H, W, 4) image, both sizes powers of two >= 4: (H x W, 4)."""
    t = np.asarray(texels); h, w = t.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((h * w, t.shape[2]), dtype=t.dtype)
    out[((y // 4) * (w // 4) + x // 4) * 16 + (y % 4) * 4 + x % 4] = t
    return out


def can_tile(texels):
    h, w = np.asarray(texels).shape[:2]
    return w >= 4 and h >= 4 and (w & (w - 1)) == 0 and (h & (h - 1)) == 0


def sample(sky, u, v, du, dv, mutate=None):
    """(E3, S:57, 73) LINEAR / WRAP sample of level 0 of the sky's texture, whatever levels it has: the uv error enters through the texels' local differences
    (tests/sampler_rule.py evaluates the corners of the box).  Returns four F; no finite bound where the uv has none."""
    import sampler_rule as SR
    tex = np.asarray(sky["texels"])
    if mutate == "tile_row_stride" and sky.get("tiled") and can_tile(tex):
        h, w = tex.shape[:2]
        y, x = np.mgrid[0:h, 0:w]
        tex = tile(tex)[tiled_index(x, y, w, h, wrong_pitch=True)]
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    du, dv = np.broadcast_to(du, u.shape), np.broadcast_to(dv, u.shape)
    ok = np.isfinite(du) & np.isfinite(dv)
    zero = np.zeros((len(u), 2))
    addr = SR.CLAMP if mutate == "clamp_instead_of_wrap" else SR.WRAP
    filt = SR.POINT if mutate == "nearest_instead_of_linear" else SR.LINEAR
    r = SR.sample_grad_bounds([tex], u, v, zero, zero, filt, addr, addr, np.where(ok, du, 0.0), np.where(ok, dv, 0.0), 0.0, 8.0 * L.U)
    return [F(0.5 * (r["vmin"][:, c] + r["vmax"][:, c]), np.where(ok, 0.5 * (r["vmax"][:, c] - r["vmin"][:, c]) + 8.0 * L.U, np.inf)) for c in range(4)]


# ---- E5: ModRGBWithHSL -------------------------------------------------------------------------------------------------------------------------------------

def hue_to_rgb(hue):
    """(C:9-14) saturate(|6 h - (3, 2, 4)| x (1, -1, -1) + (-1, 2, 2)).  The hue is NOT wrapped: past 1 and below 0 the three ramps go on into their clamps."""
    h6 = _mul(hue, 6.0)
    out = []
    for k, sign, offset in ((3.0, 1.0, -1.0), (2.0, -1.0, 2.0), (4.0, -1.0, 2.0)):
        a = _abs(L.sub(h6, k))
        out.append(L.saturate(L.add(a if sign > 0 else L.neg(a), offset)))
    return out


def mod_rgb_with_hsl(rgb, mod, mutate=None):
    """(E5, C:16-43) saturate(HSLtoRGB(RGBtoHSL(rgb) + mod)).  rgb: three F; mod: three floats.

    The two orderings of RGBtoHCV (g < b; r < max(g, b)) pick the formula of the hue.  Across r = max(g, b), and across g = b where r is NOT the largest, the two
    formulas give the same hue (1/6 or 5/6; 1/2): no decision.  Across g = b UNDER A RED MAXIMUM -- the greys among them -- the hue jumps between 0 and 1, the same
    colour only where the hue is wrapped: it is not (C:12), so with a hue modifier that is not zero the result jumps too.  That is the one decision
    (`undecided`).  With a hue modifier of zero HUEtoRGB(0) = HUEtoRGB(1) and the value is continuous there as well.
    Near a grey the hue (g - b) / (6 c) is ill-conditioned; it reaches the result through (1 - |2 L - 1|) S alone, which is 0 for a grey unless the saturation
    modifier lifts it: `hue_part` is what the float32 roundings of the colour alone come to through the hue -- the hue-conditioning bound.  (What the colour inherits
    from an uncertain uv is in the result's own bound, as everywhere.)
    Returns (three F, undecided, hue_part)."""
    r, g, b = rgb
    mx, my, mz = (_f32(m) for m in mod)
    if mutate == "saturation_on_lightness":
        my, mz = mz, my
    gb = g.v < b.v                                                                                          # (C:19)
    p0, p1 = L.where(gb, b, g), L.where(gb, g, b)
    p2, p3 = np.where(gb, -1.0, 0.0), np.where(gb, 2.0 / 3.0, -1.0 / 3.0)
    rp = r.v < p0.v                                                                                         # (C:20)
    q0, q1, q3 = L.where(rp, p0, r), p1, L.where(rp, r, p0)
    q2 = np.where(rp, p3, p2)
    red_max = r.v >= p0.v - DECISION_K * (r.e + p0.e)
    undecided = (mx != 0.0) & red_max & (np.abs(g.v - b.v) < DECISION_K * (g.e + b.e))
    c = L.sub(q0, _min2(q3, q1))                                                                            # (C:21)
    h = _abs(L.add(_div(L.sub(q3, q1), L.add(_mul(c, 6.0), HSL_EPS)), F(q2, L.U * np.abs(q2))))              # (C:22)
    z = L.sub(q0, _mul(c, 0.5))                                                                             # (C:36)
    s = _div(c, L.add(L.sub(1.0, _abs(L.sub(_mul(z, 2.0), 1.0))), HSL_EPS))                                 # (C:37)
    H, S, Lg = L.add(h, mx), L.add(s, my), L.add(z, mz)                                                     # (C:42)
    if mutate == "hue_wrapped":
        H = F(H.v - np.floor(H.v), H.e)
    base = hue_to_rgb(H)                                                                                    # (C:28)
    cc = _mul(L.sub(1.0, _abs(L.sub(_mul(Lg, 2.0), 1.0))), S)                                               # (C:29)
    out = [L.saturate(L.add(_mul(L.sub(base[k], 0.5), cc), Lg)) for k in range(3)]                          # (C:30, 42)
    # the roundings of the colour alone (a sample and a product: 4 U of the largest channel) seen through the hue: d h = 4 U q0 / (6 c), d base <= 6 d h, x |cc|
    hue_part = np.minimum(6.0 * HUE_K * L.U * np.abs(q0.v) / (6.0 * np.abs(c.v) + HSL_EPS), 1.0) * np.abs(cc.v)
    return out, undecided, hue_part


# ---- E4: the colour of a sample ----------------------------------------------------------------------------------------------------------------------------

def finish(sky, tex, step=F16_STEP, mutate=None):
    """(E4, S:58-62, 74-78) rgb x skyDiffuseMultiplier, then ModRGBWithHSL where any component of skyHSLModifier is not zero; alpha is the texel's.  -0.0 is zero:
    `any()` tests != 0, and a modifier of (-0.0, -0.0, -0.0) leaves the block off.  tex: four F.  step: half a storage step of the image the colour lands in, as a
    function of the value: a colour whose hue-conditioning bound is wider than that is claimed nowhere (an infinite bound).  Returns four F."""
    mult = [_f32(m) for m in sky["multiplier"]]
    mod = [_f32(m) for m in sky["hsl"]]
    on = any(m != 0.0 for m in mod) or mutate == "hsl_when_zero"
    if mutate == "multiplier_after_hsl" and on:
        rgb, und, part = mod_rgb_with_hsl(tex[:3], mod, mutate)
        rgb = [_mul(rgb[c], mult[c]) for c in range(3)]
    else:
        rgb = [_mul(tex[c], mult[c]) for c in range(3)]
        und = np.zeros(rgb[0].v.shape, dtype=bool); part = np.zeros(rgb[0].v.shape)
        if on:
            rgb, und, part = mod_rgb_with_hsl(rgb, mod, mutate)
    wide = und | (part > step(np.stack([c.v for c in rgb]).max(axis=0)))
    rgb = [F(c.v, np.where(wide, np.inf, c.e)) for c in rgb]
    alpha = _mul(tex[3], mult[2]) if mutate == "alpha_modified" else tex[3]
    return rgb + [alpha]


def plane_colour(sky, d, step=F16_STEP):
    """(S:71-85) SampleSkyPlane of ray directions (three F): four F."""
    m = sky.get("mutate")
    u, v, du, dv = fake_envmap_uv(d, 0.0 if m == "yaw_offset_ignored" else sky["yawOffset"], m)
    return finish(sky, sample(sky, u, v, du, dv, m), step, m)


def screen_colour(sky, camera, px, py, step=UNORM8_STEP):
    """(S:54-69) SampleSky2D of pixels: four F."""
    m = sky.get("mutate")
    u, v, du, dv = sky_plane_uv(camera, px, py, sky["yawOffset"], m)
    return finish(sky, sample(dict(sky, tiled=False), u, v, du, dv, m), step, m)


def background_yaw_offset(sky):
    """(S:91-93) the background image is looked up with a yaw offset of 0, whatever the sky's."""
    return sky["yawOffset"] if sky.get("mutate") == "yaw_offset_on_background" else 0.0


# ---- E6: sky over background -------------------------------------------------------------------------------------------------------------------------------

def over_background(bg, colour, mutate=None):
    """(E6) lerp(background, sky.rgb, sky.a) as every ray-gen shader writes it.  bg: three F; colour: four F.  Where sky.a >= 1 a side may return sky.rgb itself
    instead of (sky - bg) + bg: one rounding of the value, already in lerp's bound and added once more."""
    a = colour[3]
    if mutate == "sky_alpha_ignored":
        return list(colour[:3])
    out = []
    for c in range(3):
        x = L.lerp(bg[c], colour[c], a)
        x = F(x.v, x.e + np.where(a.v >= 1.0, L.U * np.abs(colour[c].v), 0.0))
        if mutate == "shortcut_below_one":
            x = L.where(a.v >= 0.5, colour[c], x)
        out.append(x)
    return out
