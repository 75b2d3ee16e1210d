"""The GI bounce of one frame as a rule in numpy float64 (rules I1-I12).  TEST INFRASTRUCTURE.

`indirect_kernel`, the wavefront chain `bounce_trace_* -> bounce_hit -> bounce_miss -> bounce_resolve` and `second_bounce_radiance` (csrc/passes.hip, passes_simple.hip) and
their C restatement `pass_indirect` / `gi_ray_radiance` in oracle/oracle_render.c were written from the same HLSL by the same hand.  This module states the operation a third
time, from its meaning (IndirectRayGen.hlsl:18-29, 31-137; DESIGN.md B1-B3 for the second bounce), in float64, with the `F` arithmetic of
tests/light_rule.py: every value carries a first-order bound on what a float32 evaluation may differ by, every discrete decision is taken on the value, and a pixel whose
decision has a margin below DECISION_K x the error of its two sides is reported undecided instead of guessed.  It imports nothing from oracle/ and nothing from the library.

The rule reads what is STORED -- SHADING_POSITION (float32), SHADING_NORMAL (f16 values), INSTANCE_ID, and IMAGE_BACKGROUND where the scene has a background instance --
and the scene as the host sent it.  It predicts INDIRECT_LIGHT_RAW (rgb and alpha) and GI_MOMENTS of a frame WITHOUT history (giReproject = 0: the denoiser is off).

Reference lines cited as (I:n) are IndirectRayGen.hlsl, (R:n) Random.hlsli, (S:n) BgSky.hlsli, (B:n) BlueNoise.hlsli.

Temporal reprojection -- frames WITH history -- is held by tests/temporal_rule.py (rules N1-N8), which takes this rule's frame as its fresh sample.
Out of scope: the SVGF guide and input folds of the resolve kernel, normal and specular maps at the bounce hit, hit lists past 16
entries, primary_spp > 1.
"""
import math

import numpy as np

import light_rule as L
import mirror_rule as M
import sky_rule as S
from light_rule import F
from sky_rule import fake_envmap_uv                             # (S:14-18) one definition: the background image takes it with a yaw offset of 0

EPSILON = L.EPSILON
DECISION_K = L.DECISION_K
SINCOS_ERR = 6.2e-8                                  # direction spec D1: |sin, cos of 2 pi u as both sides evaluate them - the real ones|
LUMA = [float(np.float32(x)) for x in (0.2126, 0.7152, 0.0722)]
SNORM16 = 32767.0

MUTATIONS = ("slice_from_zero", "bn_no_xmod", "uniform_weighting", "tangent_swapped", "no_depth_bias", "light_view_from_eye", "no_shadow_ray", "no_self_light",
             "no_gi_in_base", "incoming_without_no_gi", "albedo_unweighted", "sky_unweighted", "diffuse_strength_on_sky", "pick_per_sample", "second_from_first_origin",
             "second_on_first_slice", "moments_of_mean", "state_first_hit")


# ---- I2: the slice of a sample, I9: of its second bounce --------------------------------------------------------------------------------------------

def sample_slice(frame_count, s, n, mutate=None):
    """Blue-noise slice of sample s = n .. 1 of n (I:59-61): frameCount + s * (64 / n); light_rule.blue_noise takes it mod 64."""
    mult = 64 // n
    return frame_count + ((s - 1) if mutate == "slice_from_zero" else s) * mult


def second_slice(first, n, mutate=None):
    """(B1) half-way to the next sample's slice, the next slice when the samples' slices are adjacent."""
    mult = 64 // n
    return first if mutate == "second_on_first_slice" else first + (mult // 2 if mult > 1 else 1)


def noise(table, px, py, frame, channel, xmod=True):
    """light_rule.blue_noise with the ends of the range exact: byte 255 is 1.0 whether it is divided by 255 or multiplied by the float32 1 / 255 (255 x 0.0039215688 =
    1.00000006 rounds to 1), as a UNORM8 fetch gives it; byte 0 is 0.  (A sample with bn.x = 1 leaves ALONG the surface: sqrt(max(0, 1 - 1)) = 0.)"""
    f = L.blue_noise(table, px, py, frame, channel, xmod)
    return F(f.v, np.where(f.v == 1.0, 0.0, f.e))


# ---- I3: the direction ------------------------------------------------------------------------------------------------------------------------------

def perpendicular_vector(n):
    """(R:41-48) cross(u, axis): axis x where |x| is strictly the smallest, else y where |y| < |z|, else z.  Each comparison is a decision with a margin (between float32
    values without an error of their own -- a stored normal -- it is exact: a difference of two floats is negative only when the first is smaller).
    Returns (three F, undecided)."""
    a = [F(np.abs(c.v), c.e) for c in n]
    und = np.zeros(a[0].v.shape, dtype=bool)

    def less(p, q):
        nonlocal und
        und = und | (np.abs(p.v - q.v) < DECISION_K * (p.e + q.e))
        return p.v < q.v
    xm = less(a[0], a[1]) & less(a[0], a[2])
    ym = less(a[1], a[2]) & ~xm
    zm = ~(xm | ym)
    axis = [F(xm.astype(np.float64)), F(ym.astype(np.float64)), F(zm.astype(np.float64))]
    return L.cross3(n, axis), und


def bounce_direction(n, bn_x, bn_y, mutate=None):
    """(I:18-29) bitangent = perpendicular(n); tangent = bitangent x n; r = sqrt(bn.x); phi = 2 pi bn.y; d = (t r cos phi + b r sin phi) + n sqrt(max(0, 1 - bn.x)).
    Sine and cosine are the real ones, direction spec D1's error in their bound.  n: three F; bn_x, bn_y: F.  Returns (three F, undecided)."""
    b, und = perpendicular_vector(n)
    t = L.cross3(b, n)
    if mutate == "tangent_swapped":
        t, b = b, t
    r = bn_x if mutate == "uniform_weighting" else L.sqrt(bn_x)
    phi = 2.0 * math.pi * bn_y.v
    # d phi = 2 pi d bn.y; the byte / 255 carries 2 U of its value
    cs = F(np.cos(phi), SINCOS_ERR + 2.0 * math.pi * bn_y.e)
    sn = F(np.sin(phi), SINCOS_ERR + 2.0 * math.pi * bn_y.e)
    up = L.sqrt(L.fmax(L.sub(1.0, bn_x), 0.0))
    rc, rs = L.mul(r, cs), L.mul(r, sn)
    return [L.add(L.add(L.mul(t[c], rc), L.mul(b[c], rs)), L.mul(n[c], up)) for c in range(3)], und


# ---- I8: the sky term -------------------------------------------------------------------------------------------------------------------------------

def background_envmap(image, d, yaw_offset=0.0):
    """(S:91-93) LINEAR / WRAP level-0 sample of the stored IMAGE_BACKGROUND ((H, W, 4) bytes) at fake_envmap_uv(d) -- sky_rule's, with a yaw offset of 0 whatever the
    sky's (only a wrong variant passes another): the uv error enters through the texels' local differences (tests/sampler_rule.py evaluates the corners of the box).
    Returns three F."""
    import sampler_rule as SR
    u, v, du, dv = fake_envmap_uv(d, yaw_offset)
    ok = np.isfinite(du) & np.isfinite(dv)
    zero = np.zeros((len(u), 2))
    r = SR.sample_grad_bounds([np.asarray(image)], u, v, zero, zero, SR.LINEAR, SR.WRAP, SR.WRAP, np.where(ok, du, 0.0), np.where(ok, dv, 0.0), 0.0, 8.0 * L.U)
    return [F(0.5 * (r["vmin"][:, c] + r["vmax"][:, c]), np.where(ok, 0.5 * (r["vmax"][:, c] - r["vmin"][:, c]) + 8.0 * L.U, np.inf)) for c in range(3)]


def sky_term(scene, d):
    """(I:82-84) lerp(background_envmap(d), sky.rgb, sky.a): 0 without a background instance.  `scene["sky"]` is a sky description (tests/sky_rule.py: the plane is
    sampled in the ray's direction, E1-E6), or one constant texel value with alpha `skyAlpha` (1 with a sky plane, 0 without)."""
    n = len(d[0].v)
    sky = scene["sky"]
    offset = S.background_yaw_offset(sky) if S.described(sky) else 0.0
    bg = background_envmap(scene["background"], d, offset) if scene.get("background") is not None else [F(np.zeros(n)) for _ in range(3)]
    if S.described(sky):
        return S.over_background(bg, S.plane_colour(sky, d), sky.get("mutate"))
    a = float(scene.get("skyAlpha", 0.0))
    return [L.lerp(bg[c], scene["sky"][c], a) for c in range(3)]


# ---- I4-I5: the hit list of a ray and its resolve ---------------------------------------------------------------------------------------------------

def _norm_e(fs):
    return np.sqrt(sum(np.asarray(c.e, dtype=np.float64) ** 2 for c in fs))


def _settled_normal(nrm):
    """The hit record's normal is SNORM16 (mirror_rule.hit_normals keeps the unrounded value and adds half a step).  Where the unrounded value lies within its own error
    of a representable one -- the axis-aligned normal of a flat face -- the rounding changes nothing: that value, twice that error."""
    out = []
    for c in nrm:
        pre = np.maximum(np.asarray(c.e, dtype=np.float64) - M.SNORM16_HALF_STEP, 0.0)
        k = np.rint(c.v * SNORM16)
        exact = np.abs(c.v * SNORM16 - k) <= pre * SNORM16
        out.append(F(np.where(exact, k / SNORM16, c.v), np.where(exact, 2.0 * pre, c.e)))
    return out


def resolve(scene, origin, direction, mutate=None):
    """(I:86-113) the hit list of every ray (mirror_rule.hit_lists: tmin 0.1, front faces unless culling is off, order by t - depthBias) and the front-to-back loop over
    it: a hit contributes when resColor.a * alpha >= 1e-6, the loop ends when resColor.a <= 1e-6; position, normal, specular and instance id are those of the LAST
    contributing hit.  origin, direction: three F (their own errors widen the margins of the list).  Returns a dict of per-ray results."""
    n = len(origin[0].v)
    o_v = np.stack([c.v for c in origin], axis=-1); d_v = np.stack([c.v for c in direction], axis=-1)
    why = {k: np.zeros(n, dtype=bool) for k in ("hit", "order", "facing", "gate", "tie")}
    oe, de = _norm_e(origin), np.stack([np.broadcast_to(c.e, c.v.shape) for c in direction], axis=-1)
    finite = np.isfinite(oe) & np.isfinite(de).all(axis=-1)
    why["hit"] |= ~finite
    hl = M.hit_lists(scene, o_v, d_v, origin_e=np.where(finite, oe, 0.0), direction_e=np.where(finite[:, None], de, 0.0))
    count = hl["count"]; why["hit"] |= ~hl["decided"]
    hits = int(count.max()) if n else 0
    assert hits <= M.MAX_HITS, "the hit list past 16 entries is out of scope"
    inst_of_tri = M.scene_triangles(scene)[3]
    mats = scene["instances"]
    tab = lambda key: np.asarray([m["material"][key] for m in mats], dtype=np.float64)
    culled_of = np.asarray([bool(I["cull"]) for I in mats])
    res_rgb = [F(np.zeros(n)) for _ in range(3)]; res_a = F(np.ones(n))
    st_pos = [F(np.zeros(n)) for _ in range(3)]; st_nrm = [F(np.zeros(n)) for _ in range(3)]; st_spec = [F(np.zeros(n)) for _ in range(3)]
    st_id = np.full(n, -1, dtype=np.int64); contributing = np.zeros(n, dtype=np.int64)
    alive = count > 0
    for m in range(hits):
        has = alive & (count > m)
        if not has.any():
            break
        rows = np.nonzero(has)[0]
        g = lambda k: hl[k][rows, m]
        if hits > m + 1:                                          # the order of two hits: separated by more than their errors
            nxt = count[rows] > m + 1
            gap = np.where(nxt, hl["key"][rows, m + 1] - hl["key"][rows, m], np.inf)
            why["order"][rows] |= gap <= hl["key_e"][rows, m] + np.where(nxt, hl["key_e"][rows, m + 1], 0.0)
        tri = g("tri").astype(np.int64); inst = inst_of_tri[tri]
        culled = culled_of[inst]
        why["facing"][rows] |= ~culled & ~g("front_decided").astype(bool)
        col, tie, _ = M.hit_colours(scene, tri, g("u"), g("v"), g("du"), g("dv"))
        why["tie"][rows] |= tie
        h_alpha, tie = M.unorm8(tab("solidAlphaMultiplier")[inst]); why["tie"][rows] |= tie
        ra = M.take(res_a, rows)
        contrib = L.mul(ra, h_alpha)
        why["gate"][rows] |= np.abs(contrib.v - EPSILON) < DECISION_K * contrib.e
        passes = contrib.v >= EPSILON                                                                              # (I:96)
        # (I:98) origin + direction * ((t - bias) + bias)
        bias = tab("depthBias")[inst]
        tF = F(g("t"), g("dt") + 2.0 * L.U * np.abs(g("t"))) if mutate != "no_depth_bias" else F(g("t") - bias, g("dt") + 2.0 * L.U * np.abs(g("t")))
        d_r = [M.take(c, rows) for c in direction]; o_r = [M.take(c, rows) for c in origin]
        pos = L.add3(o_r, L.scale3(d_r, tF))
        nrm = M.hit_normals(scene, tri, g("u"), g("v"), g("du"), g("dv"), g("front").astype(bool) | culled)
        spec = [L.mul(F(np.asarray([m_["material"]["specularColor"][c] for m_ in mats], dtype=np.float64)[inst]), 1.0) for c in range(3)]
        keeps = passes & (st_id[rows] < 0) if mutate == "state_first_hit" else passes
        for c in range(3):
            r_c = M.take(res_rgb[c], rows)
            res_rgb[c] = M.put(res_rgb[c], has, L.where(passes, L.add(r_c, L.mul(col[c], contrib)), r_c))           # (I:102)
            st_pos[c] = M.put(st_pos[c], has, L.where(keeps, pos[c], M.take(st_pos[c], rows)))
            st_nrm[c] = M.put(st_nrm[c], has, L.where(keeps, nrm[c], M.take(st_nrm[c], rows)))
            st_spec[c] = M.put(st_spec[c], has, L.where(keeps, spec[c], M.take(st_spec[c], rows)))
        st_id[rows] = np.where(keeps, inst, st_id[rows])
        contributing[rows] += passes
        ra_new = L.where(passes, L.mul(ra, L.sub(1.0, h_alpha)), ra)                                               # (I:103)
        res_a = M.put(res_a, has, ra_new)
        why["gate"][rows] |= passes & (np.abs(ra_new.v - EPSILON) < DECISION_K * ra_new.e)
        stop = np.zeros(n, dtype=bool); stop[rows] = ra_new.v <= EPSILON                                           # (I:110)
        alive = alive & ~stop
    return dict(rgb=res_rgb, a=res_a, pos=st_pos, nrm=st_nrm, spec=st_spec, id=st_id, contributing=contributing, count=count, why=why)


# ---- I6: the light at the hit -----------------------------------------------------------------------------------------------------------------------

class _GuardedShadows:
    """A shadow test for rays whose origin is itself off by up to `radius` (a second bounce's hit): clear or occluded only if the ray and its six copies moved by
    3 x radius along the axes (an octahedron that holds the cube of side 2 x radius) agree; anything else is not decided."""

    def __init__(self, inner, positions, radius):
        self.inner = inner
        self.radius = {}
        for p, r in zip(np.ascontiguousarray(positions), radius):
            k = p.tobytes(); self.radius[k] = max(self.radius.get(k, 0.0), float(r))

    def __call__(self, origin, direction, tmin, tmax, tmin_e, tmax_e):
        r = 3.0 * np.asarray([self.radius[p.tobytes()] for p in np.ascontiguousarray(origin)])
        out = self.inner(origin, direction, tmin, tmax, tmin_e, tmax_e)
        ok = np.isfinite(r)
        for axis in range(3):
            for sign in (-1.0, 1.0):
                o = origin.copy(); o[:, axis] += sign * np.where(ok, r, 0.0)
                out = np.where(self.inner(o, direction, tmin, tmax, tmin_e, tmax_e) == out, out, -1)
        return np.where(ok, out, -1).astype(np.int8)


def lights(scene, R, direction, px, py, pick_frame, guarded, mutate=None):
    """(I:118) ComputeLightsRandom(pixel, rayDirection = the BOUNCE direction, the resolved surface, maxLightCount 1, checkShadows true) + selfLight, through
    light_rule.light_loop; the pick's random number is slice frameCount + 0 at the pixel -- the same for every sample and bounce of the pixel.
    Returns (three F for every ray, undecided by kind, rays with a surface, rays whose drawn light is shadowed, rays with a drawn light)."""
    n = len(R["id"])
    have = R["id"] >= 0
    idx = np.nonzero(have)[0]
    light = [F(np.zeros(n)) for _ in range(3)]
    why = {k: np.zeros(n, dtype=bool) for k in ("admission", "walk", "shadow", "bound")}
    shadowed, drawn = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    if not len(idx):
        return light, why, have, shadowed, drawn
    ids = R["id"][idx]
    mats = [I["material"] for I in scene["instances"]]
    tab = lambda key: np.asarray([m[key] for m in mats], dtype=np.float64)[ids]
    pos = [M.take(c, idx) for c in R["pos"]]
    view = [M.take(c, idx) for c in direction]
    if mutate == "light_view_from_eye":
        view = L.sub3(pos, [F(np.full(len(idx), float(scene["eye"][c]))) for c in range(3)])
    shadow = scene["shadow"]
    if guarded:
        pv = np.stack([c.v for c in pos], axis=-1)
        shadow = _GuardedShadows(shadow, pv, np.max(np.stack([np.broadcast_to(c.e, c.v.shape) for c in pos], axis=-1), axis=-1))
    st = {"position": pos, "normal": [M.take(c, idx) for c in R["nrm"]], "specular": [M.take(c, idx) for c in R["spec"]], "rayDirection": view,
          "px": px[idx], "py": py[idx], "bluenoise": scene["bluenoise"], "frameCount": int(pick_frame), "diSamples": int(scene["diSamples"]), "shadow": shadow,
          "checkShadows": mutate != "no_shadow_ray", "ignoreNormalFactor": tab("ignoreNormalFactor"), "specularExponent": tab("specularExponent"),
          "shadowRayBias": tab("shadowRayBias")}
    mask = np.asarray([int(m["lightGroupMaskBits"]) for m in mats], dtype=np.uint32)[ids]
    res, w, _, draws, _, in_shadow = L.light_loop(st, mask, scene["lights"], 1)
    if mutate != "no_self_light":
        self_light = np.asarray([m["selfLight"] for m in mats], dtype=np.float64)[ids]
        res = [L.add(a, F(self_light[:, c])) for c, a in enumerate(res)]
    for c in range(3):
        light[c] = M.put(light[c], have, res[c])
    for k in why:
        why[k][idx] = w[k]
    shadowed[idx] = in_shadow; drawn[idx] = draws > 0
    return light, why, have, shadowed, drawn


# ---- I7, I9: the radiance of a ray ------------------------------------------------------------------------------------------------------------------

def ray_radiance(scene, origin, direction, px, py, slice_, more, second, counts, mutate=None):
    """(I:81-123; B1-B3) what one GI ray brings back: ambientBase + colour (1 - remaining) (incoming + light) giDiffuseStrength + sky(d) giSkyStrength remaining.
    incoming = ambientBase + ambientNoGI, or (more > 0) the radiance of ONE further ray from the resolved position about the resolved normal.
    Returns (three F, undecided (n,))."""
    n = len(px)
    R = resolve(scene, origin, direction, mutate)
    pick_frame = slice_ if mutate == "pick_per_sample" else scene["frameCount"]
    if int(scene["diSamples"]) > 0:
        assert mutate != "pick_per_sample", "with diSamples > 0 the variant would move the light's disc samples as well"
    light, lwhy, have, shadowed, drawn = lights(scene, R, direction, px, py, pick_frame, second, mutate)
    und = np.zeros(n, dtype=bool)
    for k, x in list(R["why"].items()) + [("light_" + k_, x_) for k_, x_ in lwhy.items()]:
        und |= x
        if x.any():
            counts["undecided_" + k] = counts.get("undecided_" + k, 0) + int(x.sum())
    base = [float(scene["ambientBase"][c]) for c in range(3)]
    no_gi = [float(scene["ambientNoGI"][c]) for c in range(3)]
    incoming = [F(np.full(n, base[c])) if mutate == "incoming_without_no_gi" else L.add(F(np.full(n, base[c])), no_gi[c]) for c in range(3)]
    if more > 0 and have.any():                                                                                 # (B1, B2)
        idx = np.nonzero(have)[0]
        nrm = _settled_normal([M.take(c, idx) for c in R["nrm"]])
        nxt = second_slice(slice_, int(scene["giSamples"]), mutate)
        xmod = mutate != "bn_no_xmod"
        d2, dund = bounce_direction(nrm, noise(scene["bluenoise"], px[idx], py[idx], nxt, 0, xmod), noise(scene["bluenoise"], px[idx], py[idx], nxt, 1, xmod), mutate)
        o2 = [M.take(c, idx) for c in (origin if mutate == "second_from_first_origin" else R["pos"])]
        rad2, und2 = ray_radiance(scene, o2, d2, px[idx], py[idx], nxt, more - 1, True, counts, mutate)
        und[idx] |= und2 | dund
        incoming = [M.put(incoming[c], have, rad2[c]) for c in range(3)]
    covered = L.sub(1.0, R["a"])
    sky = sky_term(scene, direction)
    gd, gs = float(scene["giDiffuseStrength"]), float(scene["giSkyStrength"])
    out = []
    for c in range(3):
        start = L.add(F(np.full(n, base[c])), no_gi[c]) if mutate == "no_gi_in_base" else F(np.full(n, base[c]))            # (I:116)
        albedo = R["rgb"][c] if mutate == "albedo_unweighted" else L.mul(R["rgb"][c], covered)
        bounce = L.mul(L.mul(albedo, L.add(incoming[c], light[c])), gd)                                         # (I:119)
        res = L.where(have, L.add(start, bounce), start)
        weight = L.mul(gs, F(np.ones(n)) if mutate == "sky_unweighted" else R["a"])
        if mutate == "diffuse_strength_on_sky":
            weight = L.mul(weight, gd)
        term = L.mul(sky[c], weight)                                                                            # (I:123) either order of the two products: one more rounding
        if S.described(scene["sky"]):                                                                           # nothing remains: the sky is not seen, whatever bound its colour has
            term = L.where((weight.v == 0.0) & (weight.e == 0.0), 0.0, term)
        out.append(L.add(res, F(term.v, term.e + L.U * np.abs(term.v))))
    sky_seen = (np.stack([np.abs(s.v) for s in sky], axis=-1).max(axis=-1) > 0.0) & (R["a"].v > 0.0)
    if scene.get("skySeen") is not None:
        scene["skySeen"][py[sky_seen], px[sky_seen]] = True
    for k, x in (("hit", R["count"] > 0), ("miss", R["count"] == 0), ("lit", drawn & ~shadowed), ("shadowed", shadowed), ("two_contributing", R["contributing"] >= 2),
                 ("sky", sky_seen)):
        counts[k] = counts.get(k, 0) + int(x.sum())
    return out, und


# ---- the pass (I1, I10-I12) -------------------------------------------------------------------------------------------------------------------------

def _f16_bound(v, e):
    return e + np.maximum(L.F16_HALF_STEP * (np.abs(v) + e), L.F16_FLOOR)


def indirect(scene, position, normal, instance_id, mutate=None):
    """IndirectRayGen for every pixel of a frame without history.  position, normal: (H, W, >= 3) as stored; instance_id: (H, W) int.

    scene: instances, lights, ambientBase, ambientNoGI, sky (a description for tests/sky_rule.py, or the one constant term), bluenoise, frameCount, diSamples, shadow as tests/mirror_rule.py reads them, and skyAlpha (1 with a sky plane,
    else 0), skySeen (optional (H, W) bool array: the rule marks the pixels one of whose rays sees the sky), background (the stored IMAGE_BACKGROUND or None), giSamples, giBounces, giDiffuseStrength, giSkyStrength, eye (only a wrong variant reads it).
    Returns dict: value, bound (H, W, 4) of INDIRECT_LIGHT_RAW (alpha = giSamples on a surface, 0 elsewhere: bound 0), moments, moments_bound (H, W, 2) of GI_MOMENTS,
    decided (H, W), surface (H, W), info (counts over the rays of the frame, undecided pixels)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    instance_id = np.asarray(instance_id); h, w = instance_id.shape
    ns, bounces = int(scene["giSamples"]), int(scene["giBounces"])
    value = np.zeros((h, w, 4)); bound = np.zeros((h, w, 4)); moments = np.zeros((h, w, 2)); moments_bound = np.zeros((h, w, 2))
    ambient = [L.add(float(scene["ambientBase"][c]), float(scene["ambientNoGI"][c])) for c in range(3)]                   # (I:135)
    for c in range(3):
        value[..., c] = ambient[c].v; bound[..., c] = _f16_bound(ambient[c].v, ambient[c].e)
    surface = (instance_id >= 0) & (ns > 0)                                                                      # (I:35)
    decided = np.ones((h, w), dtype=bool)
    counts = {}
    if not surface.any():
        return dict(value=value, bound=bound, moments=moments, moments_bound=moments_bound, decided=decided, surface=surface, info=dict(counts=counts, undecided=0))
    py, px = np.nonzero(surface)
    n = len(px)
    origin = L.vec(np.asarray(position, dtype=np.float64)[surface][:, :3])
    nrm = L.vec(np.asarray(normal, dtype=np.float64)[surface][:, :3])
    acc = [F(np.zeros(n)) for _ in range(3)]
    sum_l, sum_l2 = F(np.zeros(n)), F(np.zeros(n))
    und = np.zeros(n, dtype=bool)
    xmod = mutate != "bn_no_xmod"
    for hist, s in enumerate(range(ns, 0, -1), start=1):                                                         # (I:58-60): maxSamples counts down, the history up
        sl = sample_slice(int(scene["frameCount"]), s, ns, mutate)
        d, dund = bounce_direction(nrm, noise(scene["bluenoise"], px, py, sl, 0, xmod), noise(scene["bluenoise"], px, py, sl, 1, xmod), mutate)
        rad, rund = ray_radiance(scene, origin, d, px, py, sl, 1 if bounces >= 2 else 0, False, counts, mutate)
        und |= dund | rund
        inv = L.rcp(F(np.full(n, float(hist))))                                                                  # (I:126-127): a 1-ulp reciprocal
        acc = [L.lerp(acc[c], rad[c], inv) for c in range(3)]
        lum = L.add(L.add(L.mul(rad[0], LUMA[0]), L.mul(rad[1], LUMA[1])), L.mul(rad[2], LUMA[2]))
        sum_l = L.add(sum_l, lum); sum_l2 = L.add(sum_l2, L.mul(lum, lum))
    if mutate == "moments_of_mean":
        lum = L.add(L.add(L.mul(acc[0], LUMA[0]), L.mul(acc[1], LUMA[1])), L.mul(acc[2], LUMA[2]))
        sum_l = L.mul(lum, float(ns)); sum_l2 = L.mul(L.mul(lum, lum), float(ns))
    m1, m2 = L.div(sum_l, float(ns)), L.div(sum_l2, float(ns))                                                    # alphaM = min(n / n, 1) = 1: lerp(0, x, 1) = x
    v = np.stack([c.v for c in acc], axis=-1); e = np.stack([np.broadcast_to(c.e, c.v.shape) for c in acc], axis=-1)
    value[surface] = np.concatenate([v, np.full((n, 1), float(ns))], axis=-1)
    bound[surface] = np.concatenate([_f16_bound(v, e), np.zeros((n, 1))], axis=-1)
    mv = np.stack([m1.v, m2.v], axis=-1); me = np.stack([m1.e, m2.e], axis=-1)
    moments[surface] = mv; moments_bound[surface] = me + 2.0 * L.U * np.abs(mv)
    und |= ~np.isfinite(bound[surface]).all(axis=-1) | ~np.isfinite(moments_bound[surface]).all(axis=-1)          # no finite bound: not claimed; a NaN is claimed, and wrong
    decided[surface] = ~und
    return dict(value=value, bound=bound, moments=moments, moments_bound=moments_bound, decided=decided, surface=surface,
                info=dict(counts=counts, undecided=int(und.sum())))


def compare(stored, stored_moments, rule):
    """(largest ratio, mean ratio, pixels outside) of a stored INDIRECT_LIGHT_RAW and GI_MOMENTS against a rule result: rgb and moments within the bound at every decided
    pixel (ratio < 1); alpha equal at every pixel."""
    dev = np.concatenate([np.abs(np.asarray(stored, dtype=np.float64)[..., :3] - rule["value"][..., :3]), np.abs(np.asarray(stored_moments, dtype=np.float64) - rule["moments"])], axis=-1)
    b = np.concatenate([rule["bound"][..., :3], rule["moments_bound"]], axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(dev == 0.0, 0.0, dev / b)
    ratio = np.where(np.isnan(ratio), np.inf, ratio).max(axis=-1)
    ok = rule["decided"]
    bad = ok & (ratio >= 1.0)
    bad |= np.asarray(stored)[..., 3] != rule["value"][..., 3]
    return float(ratio[ok].max()), float(ratio[ok].mean()), bad
