"""Direct lighting of one frame as a rule in numpy float64 (rules L1-L9).  TEST INFRASTRUCTURE.

The light loop (`light_intensity_simple`, `compute_light`, `compute_lights_random` in csrc/shade.h, `direct_light_pixel` in
csrc/passes.hip) and its C restatement in oracle/oracle_shade.c were both written from the same HLSL.  This module states the same
operation a third time, from its meaning (SURVEY.md A7, a10 and the rows around them), in float64, and carries with every value a
first-order bound on what float32 arithmetic and the device's approximate instructions may do to it.  It imports nothing from oracle/.

Every quantity is an `F`: a float64 value `v` and an absolute error bound `e` such that a float32 evaluation of the same expression
(correctly rounded +, -, *; 1-ulp rcp / rsqrt / sqrt / log2 / exp2) lies within `v +- e`.  Discrete decisions (candidate admission,
each comparison of the CDF walk, each shadow ray) are taken on `v`; where the margin of a decision is below DECISION_K times the
error of the quantities compared the pixel is reported as not decided instead of guessed.

Reference lines cited as (L:n) are Lights.hlsli, (D:n) DirectRayGen.hlsl, (B:n) BlueNoise.hlsli.
"""
import math

import numpy as np

U = 2.0 ** -24            # one correctly rounded float32 operation, relative (half an ulp)
A = 2.0 ** -23            # one ulp: the device's rcp, rsqrt, sqrt, log2, exp2 as documented
LOG_FLOOR = 2.0 ** -23    # log2's absolute error is taken as 1 ulp of the result or of 1.0, whichever is larger (no relative promise around x = 1)
CAM_K = 16                # upper estimate of the float32 roundings between the camera's parameters and rayDirection (projection, two inverses, two products)
DECISION_K = 1.5          # a decision is trusted when its margin is at least DECISION_K x the (worst-case, first-order) error of the two sides
SHADOW_K = 64             # upper estimate of the float32 roundings of a ray / triangle test, the ray's world -> object transform and its direction (L7)
MAX_LIGHTS = 16           # (L:25)
EPSILON = float(np.float32(1e-6))          # Constants.hlsli:5
RAY_MIN_DISTANCE = float(np.float32(0.1))  # Ray.hlsli:9
F16_HALF_STEP = 2.0 ** -11                 # half a step of an RGBA16F channel, relative
F16_FLOOR = 2.0 ** -25                     # half a step among f16 subnormals

MUTATIONS = ("select_slot_plus_one", "sample_slot_up", "invprob_always", "not_zeroed", "radius_at_zero", "offset_added",
             "tmin_no_bias", "ndotl_unclamped", "raydir_normalised", "eye_spec_unsaturated", "cap_scanned", "bn_no_xmod")


# ---- values with an error bound ------------------------------------------------------------------------------------------------------------

class F:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)


def _f(x):
    return x if isinstance(x, F) else F(x)


def add(a, b):
    a, b = _f(a), _f(b)
    v = a.v + b.v
    return F(v, a.e + b.e + U * np.abs(v))


def neg(a):
    return F(-a.v, a.e)


def sub(a, b):
    return add(a, neg(_f(b)))


def mul(a, b):
    a, b = _f(a), _f(b)
    v = a.v * b.v
    return F(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + U * np.abs(v))


def rcp(a):
    """1-ulp reciprocal."""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = 1.0 / a.v
        lo = np.abs(a.v) - a.e
        e = np.where(lo > 0.0, a.e / (np.abs(a.v) * np.where(lo > 0.0, lo, 1.0)), np.inf) + A * np.abs(v)
    return F(v, e)


def div(a, b):
    return mul(a, rcp(_f(b)))


def sqrt(a):
    v = np.sqrt(np.maximum(a.v, 0.0))
    hi, lo = np.sqrt(np.maximum(a.v + a.e, 0.0)), np.sqrt(np.maximum(a.v - a.e, 0.0))
    return F(v, np.maximum(hi - v, v - lo) + A * v)


def rsqrt(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = 1.0 / np.sqrt(a.v)
        lo = a.v - a.e
        e = np.where(lo > 0.0, 1.0 / np.sqrt(np.where(lo > 0.0, lo, 1.0)) - v, np.inf) + A * v
    return F(v, e)


def fmax(a, c):
    """max with a constant: the clamped ends of v +- e (no error is left where the whole range lies under the constant)."""
    v = np.maximum(a.v, c)
    return F(v, np.maximum(np.maximum(a.v + a.e, c) - v, v - np.maximum(a.v - a.e, c)))


def saturate(a):
    v = np.clip(a.v, 0.0, 1.0)
    return F(v, np.maximum(np.clip(a.v + a.e, 0.0, 1.0) - v, v - np.clip(a.v - a.e, 0.0, 1.0)))


def power(a, y):
    """pow(x, y) for x >= 0, y >= 0 exact: exp2(y * log2 x), and 1 when y is 0 whatever x is (also at x = 0)."""
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), a.v.shape)
    x = np.maximum(a.v, 0.0)
    hi, lo = x + a.e, np.maximum(x - a.e, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.power(x, y)
        spread = np.maximum(np.abs(np.power(hi, y) - v), np.abs(v - np.power(lo, y)))          # the argument's own error, through the function
        lg = np.where(x > 0.0, np.abs(np.log2(np.where(x > 0.0, x, 1.0))), 0.0)
        # log2: max(A |log2 x|, LOG_FLOOR); the product y log2 x: one rounding; exp2 turns an absolute error d of its argument into a relative error ln2 d; exp2 itself: 1 ulp
        rel = math.log(2.0) * (y * np.maximum(A * lg, LOG_FLOOR) + U * y * lg) + A
    zero = y == 0.0
    return F(np.where(zero, 1.0, v), np.where(zero, 0.0, spread + rel * v * (1.0 + rel)))


def where(c, a, b):
    a, b = _f(a), _f(b)
    return F(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def vec(x):
    """(N, 3) exact values -> three F."""
    return [F(x[..., 0]), F(x[..., 1]), F(x[..., 2])]


def dot3(a, b):
    return add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))


def cross3(a, b):
    return [sub(mul(a[1], b[2]), mul(a[2], b[1])), sub(mul(a[2], b[0]), mul(a[0], b[2])), sub(mul(a[0], b[1]), mul(a[1], b[0]))]


def scale3(a, s):
    return [mul(c, s) for c in a]


def add3(a, b):
    return [add(x, y) for x, y in zip(a, b)]


def sub3(a, b):
    return [sub(x, y) for x, y in zip(a, b)]


def neg3(a):
    return [neg(c) for c in a]


def length3(a):
    return sqrt(dot3(a, a))


def normalize3(a):
    return scale3(a, rsqrt(dot3(a, a)))


def lerp(a, b, t):
    return add(a, mul(t, sub(b, a)))             # HLSL lerp


def reflect3(i, n):
    return sub3(i, scale3(n, mul(2.0, dot3(n, i))))


# ---- camera (D:23-26) ----------------------------------------------------------------------------------------------------------------------

def ray_direction(camera, normalised=False):
    """rayDirection of every pixel, (H, W, 3) float64: the far-plane target of the pixel's centre (+ jitter) taken through the inverse projection, its xyz
    taken through the inverse view as a vector.  It is not normalised (D:26)."""
    w, h = int(camera["width"]), int(camera["height"])
    fov, zn, zf = float(camera["fov"]), float(camera["near"]), float(camera["far"])
    jx, jy = camera.get("jitter", (0.0, 0.0))
    sy = 1.0 / math.tan(0.5 * fov); sx = sy / (w / h); rng = zf / (zn - zf)
    proj = np.zeros((4, 4)); proj[0, 0] = sx; proj[1, 1] = sy; proj[2, 2] = rng; proj[2, 3] = -1.0; proj[3, 2] = rng * zn       # right-handed perspective, row vectors
    proj_i = np.linalg.inv(proj); view_i = np.linalg.inv(np.asarray(camera["view"], dtype=np.float64))
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="xy")
    dx = (px + 0.5 + jx) / w * 2.0 - 1.0; dy = (py + 0.5 + jy) / h * 2.0 - 1.0
    target = np.stack([dx, -dy, np.ones_like(dx), np.ones_like(dx)], axis=-1) @ proj_i
    d = target[..., :3] @ view_i[:3, :3]
    if normalised:
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return d


# ---- blue noise (B:7-13) -------------------------------------------------------------------------------------------------------------------

def blue_noise(table, px, py, frame, channel, xmod=True):
    """Channel of the 512 x 512 RGBA8 table as value / 255: slice frame % 64 of an 8 x 8 atlas of 64 x 64 tiles, addressed by px % 64, py % 64."""
    f = int(frame) % 64
    bx = (f % 8) * 64 + (px % 64 if xmod else px)
    by = (f // 8) * 64 + py % 64
    v = table[by % 512, bx % 512, channel].astype(np.float64) / 255.0
    return F(v, 2.0 * U * v)                     # byte * (1 / 255): the constant and the product each round once


# ---- shadows: float64 brute force over world-space triangles ----------------------------------------------------------------------------------

class BruteForceShadows:
    """shadow(origin, direction, tmin, tmax, tmin_err, tmax_err) -> 1 clear, 0 occluded, -1 not decided, for opaque casters.

    Every ray is tested against every triangle (no back-face cull, L:46) in float64: with tv = o - v0, det = e1 . (d x e2), u = tv . (d x e2) / det,
    v = d . (tv x e1) / det, t = e2 . (tv x e1) / det.  A float32 test may be off by SHADOW_K roundings of the largest product in each numerator and in det (L7):
    d_u = K U (T |d| |e2| / |det| + |u|), d_v = K U (T |d| |e1| / |det| + |v|), d_t = K U (T |e1| |e2| / |det| + |t|), T = |tv| + (|o| + |v0|) / K (the
    subtraction o - v0 rounds at the size of its operands).  Occluded: some triangle has u > d_u, v > d_v, 1 - u - v > d_u + d_v and
    tmin + d_t < t < tmax - d_t.  Clear: every triangle has one of u < -d_u, v < -d_v, 1 - u - v < -(d_u + d_v), t < tmin - d_t, t > tmax + d_t."""

    def __init__(self, groups, chunk=2048):
        """groups: one (T, 3, 3) array of world-space triangles per instance.  A group is skipped for the rays whose line passes its bounding sphere at more than
        1 + 2^-10 of its radius: such a ray misses every triangle of the group by far more than the margins above."""
        self.groups = []
        for g in groups:
            t = np.asarray(g, dtype=np.float64).reshape(-1, 3, 3)
            centre = 0.5 * (t.reshape(-1, 3).min(axis=0) + t.reshape(-1, 3).max(axis=0))
            radius = np.linalg.norm(t.reshape(-1, 3) - centre, axis=1).max()
            self.groups.append((t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], centre, radius))
        self.chunk = chunk
        self.rays = 0

    def __call__(self, origin, direction, tmin, tmax, tmin_err, tmax_err):
        n = len(origin)
        self.rays += n
        occluded = np.zeros(n, dtype=bool); clear = np.ones(n, dtype=bool)
        unit = direction / np.linalg.norm(direction, axis=1, keepdims=True)
        for v0, e1, e2, centre, radius in self.groups:
            to_c = centre[None] - origin
            off = np.linalg.norm(to_c - (to_c * unit).sum(axis=1, keepdims=True) * unit, axis=1)
            near = np.nonzero(off <= radius * (1.0 + 2.0 ** -10))[0]
            for a in range(0, len(near), self.chunk):
                i = near[a:a + self.chunk]
                hit, miss = self._chunk(v0, e1, e2, origin[i], direction[i], tmin[i], tmax[i], tmin_err[i], tmax_err[i])
                occluded[i] |= hit; clear[i] &= miss
        return np.where(occluded, 0, np.where(clear, 1, -1)).astype(np.int8)

    @staticmethod
    def _chunk(v0, e1, e2, o, d, tmin, tmax, tmin_e, tmax_e):
        u, v, t, du, dv, dt, _, ok = triangle_test(v0, e1, e2, o, d)
        w = 1.0 - u - v
        lo, hi = tmin[:, None], tmax[:, None]
        lo_e, hi_e = tmin_e[:, None] + dt, tmax_e[:, None] + dt
        hit = ok & (u > du) & (v > dv) & (w > du + dv) & (t > lo + lo_e) & (t < hi - hi_e)
        miss = ok & ((u < -du) | (v < -dv) | (w < -(du + dv)) | (t < lo - lo_e) | (t > hi + hi_e))
        return hit.any(axis=1), miss.all(axis=1)


def triangle_test(v0, e1, e2, o, d):
    """Every ray (o, d: (N, 3)) against every triangle (v0, e1, e2: (T, 3)) in float64, with the margins of BruteForceShadows' docstring: returns
    (u, v, t, d_u, d_v, d_t, det, ok), each (N, T); ok is False where a quantity is not finite (a ray in the triangle's plane)."""
    l1, l2, l0 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1), np.linalg.norm(v0, axis=1)
    e1, e2 = e1[None], e2[None]
    p = np.cross(d[:, None, :], e2)
    det = np.einsum("ntk,ntk->nt", np.broadcast_to(e1, p.shape), p)
    tv = o[:, None, :] - v0[None]
    q = np.cross(tv, e1)
    T = np.linalg.norm(tv, axis=2) + (np.linalg.norm(o, axis=1)[:, None] + l0[None]) / SHADOW_K
    dl = np.linalg.norm(d, axis=1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        u = np.einsum("ntk,ntk->nt", tv, p) * inv
        v = np.einsum("nk,ntk->nt", d, q) * inv
        t = np.einsum("ntk,ntk->nt", np.broadcast_to(e2, q.shape), q) * inv
        k = SHADOW_K * U
        du = k * (T * dl * l2[None] * np.abs(inv) + np.abs(u))
        dv = k * (T * dl * l1[None] * np.abs(inv) + np.abs(v))
        dt = k * (T * l1[None] * l2[None] * np.abs(inv) + np.abs(t))
    ok = np.isfinite(u) & np.isfinite(v) & np.isfinite(t) & np.isfinite(du) & np.isfinite(dv) & np.isfinite(dt)
    return u, v, t, du, dv, dt, det, ok


# ---- the light loop ------------------------------------------------------------------------------------------------------------------------

_LIGHT_FIELDS = ("position", "diffuseColor", "attenuationRadius", "pointRadius", "specularColor", "shadowOffset", "attenuationExponent", "groupBits")


def _light_table(lights):
    t = {}
    for k in _LIGHT_FIELDS:
        t[k] = np.asarray([l[k] for l in lights], dtype=np.uint32 if k == "groupBits" else np.float64)
    return t


def _intensity_simple(L, position, normal, ignore_normal):                     # (L:54-65)
    lp = vec(L["position"])
    to_point = sub3(position, lp)
    distance = length3(to_point)
    direction = normalize3(sub3(lp, position))
    ndotl = dot3(normal, direction)                                            # not clamped here
    bias = fmax(add(lerp(ndotl, 1.0, ignore_normal), float(np.float32(0.707106))), 0.0)
    inside = fmax(sub(1.0, div(distance, L["attenuationRadius"])), 0.0)
    falloff = power(inside, L["attenuationExponent"])
    colour = add(add(F(L["diffuseColor"][..., 0]), L["diffuseColor"][..., 1]), L["diffuseColor"][..., 2])
    return mul(mul(falloff, bias), colour), inside.v <= 0.0


def _compute_light(L, st, active, mutate):                                      # (L:67-113)
    position, normal, specular, ray_dir = st["position"], st["normal"], st["specular"], st["rayDirection"]
    di_samples, frame = st["diSamples"], st["frameCount"]
    lp = vec(L["position"])
    direction = normalize3(sub3(lp, position))
    radius = L["pointRadius"] if (di_samples > 0 or mutate == "radius_at_zero") else np.zeros_like(L["pointRadius"])      # (L:75)
    perp_x = cross3(neg3(direction), [F(np.zeros_like(radius)), F(np.ones_like(radius)), F(np.zeros_like(radius))])        # (L:76): (dir.z, 0, -dir.x)
    # (L:77-79) all(perpX == 0): the light is exactly above or below the point.  Exact in float32 too: a difference of floats is 0 only when they are equal.
    straight = (L["position"][..., 0] == position[0].v) & (L["position"][..., 2] == position[2].v)
    perp_x[0] = where(straight, 1.0, perp_x[0])
    perp_y = cross3(perp_x, neg3(direction))
    max_samples = max(di_samples, 1)                                           # (L:83)
    rs = F(np.float64(1.0 / max_samples), A / max_samples)
    n = len(radius)
    lambert, shadow, spec = F(np.zeros(n)), F(np.zeros(n)), [F(np.zeros(n)) for _ in range(3)]
    undecided = np.zeros(n, dtype=bool)
    shadowed = np.zeros(n, dtype=bool)
    for k in range(max_samples):
        samples = max_samples - k                                              # counts down from maxSamples (L:84-109)
        slot = frame + (k if mutate == "sample_slot_up" else samples)         # (L:89)
        xmod = mutate != "bn_no_xmod"
        cx = sub(mul(blue_noise(st["bluenoise"], st["px"], st["py"], slot, 0, xmod), 2.0), 1.0)
        cy = sub(mul(blue_noise(st["bluenoise"], st["px"], st["py"], slot, 1, xmod), 2.0), 1.0)
        ln = sqrt(add(mul(cx, cx), mul(cy, cy)))                               # never 0: no byte / 255 is 0.5
        k_disc = mul(rcp(ln), saturate(ln))                                    # normalize(c) * saturate(length(c)) (L:90)
        cx, cy = mul(cx, k_disc), mul(cy, k_disc)
        sample_pos = add3(add3(lp, scale3(scale3(perp_x, cx), radius)), scale3(scale3(perp_y, cy), radius))       # (L:92)
        sample_dist = length3(sub3(position, sample_pos))
        sample_dir = normalize3(sub3(sample_pos, position))
        falloff = power(fmax(sub(1.0, div(sample_dist, L["attenuationRadius"])), 0.0), L["attenuationExponent"])  # (L:95)
        reflected = reflect3(neg3(sample_dir), normal)
        ndotl = dot3(normal, sample_dir)
        if mutate != "ndotl_unclamped":
            ndotl = fmax(ndotl, 0.0)                                           # (L:97)
        s_lambert = mul(lerp(ndotl, 1.0, st["ignoreNormalFactor"]), falloff)   # (L:98)
        # (L:101) origin: the position; direction: normalised; tmin = 0.1 + shadowRayBias; tmax = distance - shadowOffset
        tmin = add(RAY_MIN_DISTANCE, st["shadowRayBias"]) if mutate != "tmin_no_bias" else F(np.full(n, RAY_MIN_DISTANCE))
        tmax = sub(sample_dist, L["shadowOffset"]) if mutate != "offset_added" else add(sample_dist, L["shadowOffset"])
        sh = np.ones(n, dtype=np.int8)
        if active.any() and st.get("checkShadows", True):
            o = np.stack([c.v for c in position], axis=-1)[active]
            d = np.stack([c.v for c in sample_dir], axis=-1)[active]
            sh[active] = st["shadow"](o, d, tmin.v[active], tmax.v[active], tmin.e[active], tmax.e[active])
        undecided |= active & (sh < 0)
        shadowed |= active & (sh == 0)
        s_spec = power(fmax(saturate(mul(dot3(reflected, neg3(ray_dir)), falloff)), 0.0), st["specularExponent"])  # (L:104)
        lambert = add(lambert, mul(s_lambert, rs))                             # (L:105-107): / maxSamples
        spec = [add(a, mul(mul(c, s_spec), rs)) for a, c in zip(spec, specular)]
        shadow = add(shadow, mul(F((sh > 0).astype(np.float64)), rs))
    out = []
    for c in range(3):                                                         # (L:112)
        out.append(mul(add(mul(F(L["diffuseColor"][..., c]), lambert), mul(F(L["specularColor"][..., c]), spec[c])), shadow))
    return out, undecided, shadowed


def light_loop(st, mask_bits, lights, max_lights, mutate=None):
    """compute_lights_random (L:115-168) for n points: the candidate scan, `max_lights` draws by the CDF walk, each drawn light through _compute_light.

    st: position, normal, specular, rayDirection as three F of n values each (they may carry an error of their own); px, py (n,) int; bluenoise; frameCount;
    diSamples; ignoreNormalFactor, specularExponent, shadowRayBias (n,) float64; shadow (see BruteForceShadows); checkShadows (default True: False sends no
    shadow ray and every sample counts as clear).  mask_bits: (n,) uint32, the material's lightGroupMaskBits.
    Returns (result: three F, why: the undecided pixels by kind of decision, candidates admitted, draws made, lights whose radius the point lies beyond, in shadow)."""
    n = len(mask_bits)
    T = _light_table(lights)
    why = {k: np.zeros(n, dtype=bool) for k in ("admission", "walk", "shadow", "bound")}          # which kind of decision float32 could take the other way
    outside = np.zeros(n, dtype=np.int64)             # lights let through by the mask whose radius the pixel lies beyond

    # candidates: the first lights, up to 16 ADMITTED, whose group bits meet the material's mask and whose simple intensity is above 1e-6 (L:126-136)
    count = np.zeros(n, dtype=np.int64)
    s_int = [F(np.zeros(n)) for _ in range(MAX_LIGHTS)]
    s_idx = np.zeros((n, MAX_LIGHTS), dtype=np.int64)
    for l in range(len(lights)):
        if mutate == "cap_scanned" and l >= MAX_LIGHTS:
            break
        Ll = {k: np.broadcast_to(T[k][l], (n,) + T[k][l].shape) for k in _LIGHT_FIELDS}
        scanned = ((mask_bits & T["groupBits"][l]) != 0) & (count < MAX_LIGHTS)          # a mask of 0 admits nothing: zero from the loop (L:119)
        if not scanned.any():
            continue
        li, beyond = _intensity_simple(Ll, st["position"], st["normal"], st["ignoreNormalFactor"])
        outside += scanned & beyond
        why["admission"] |= scanned & (np.abs(li.v - EPSILON) < DECISION_K * li.e)
        admitted = scanned & (li.v > EPSILON)
        for slot in range(MAX_LIGHTS):
            here = admitted & (count == slot)
            if here.any():
                s_int[slot] = where(here, li, s_int[slot])
                s_idx[here, slot] = l
        count += admitted
    total = F(np.zeros(n))
    for slot in range(MAX_LIGHTS):
        total = where(count > slot, add(total, s_int[slot]), total)

    draws = np.minimum(count, int(max_lights))                                  # (L:139)
    use_probability = (draws == 1) if mutate != "invprob_always" else np.full(n, int(max_lights) >= 1)      # (L:145)
    remaining = total
    result = [F(np.zeros(n)) for _ in range(3)]
    in_shadow = np.zeros(n, dtype=bool)
    for s in range(int(draws.max()) if n else 0):
        active = s < draws
        slot = st["frameCount"] + s + (1 if mutate == "select_slot_plus_one" else 0)
        r = mul(blue_noise(st["bluenoise"], st["px"], st["py"], slot, 0, mutate != "bn_no_xmod"), remaining)                   # (L:147)
        chosen = np.zeros(n, dtype=np.int64)
        running = s_int[0]
        walking = active.copy()
        for k in range(MAX_LIGHTS - 1):                                          # (L:148-153): while chosen < count - 1 and r >= running
            test = walking & (chosen < count - 1)
            why["walk"] |= test & (np.abs(r.v - running.v) < DECISION_K * (r.e + running.e))
            step = test & (r.v >= running.v)
            chosen = chosen + step
            nxt = F(np.choose(chosen, [c.v for c in s_int]), np.choose(chosen, [c.e for c in s_int]))
            running = where(step, add(running, nxt), running)
            walking = step
            if not step.any():
                break
        c_int = F(np.choose(chosen, [c.v for c in s_int]), np.choose(chosen, [c.e for c in s_int]))
        c_idx = s_idx[np.arange(n), chosen]
        inv_p = where(use_probability, div(remaining, where(active, c_int, 1.0)), 1.0)                        # (L:158)
        if mutate != "not_zeroed":
            for slot_k in range(MAX_LIGHTS):                                     # (L:159)
                s_int[slot_k] = where(active & (chosen == slot_k), 0.0, s_int[slot_k])
        remaining = where(active, sub(remaining, c_int), remaining)              # (L:160)
        Lc = {k: T[k][c_idx] for k in _LIGHT_FIELDS}
        light, und, shd = _compute_light(Lc, st, active, mutate)
        why["shadow"] |= und
        in_shadow |= shd
        result = [where(active, add(a, mul(c, inv_p)), a) for a, c in zip(result, light)]                     # (L:163)

    return result, why, count, draws, outside, in_shadow


def direct_light(position, normal, specular, instance_id, materials, lights, eye_diffuse, eye_specular, max_lights, di_samples, frame_count, bluenoise, camera,
                 shadow, mutate=None):
    """resDirect of DirectRayGen for every pixel of a frame, as the RGBA16F image stores it when nothing is accumulated (w = 1; a miss is (1, 1, 1, 0), D:18-21).

    position, normal, specular: (H, W, >= 3) as stored (float32 / f16 values); instance_id: (H, W) int, < 0 for a miss; materials: per instance id a dict of the fields
    the loop reads (lightGroupMaskBits, ignoreNormalFactor, specularExponent, shadowRayBias, selfLight); lights: dicts of the RT64_LIGHT fields; camera: dict(view, fov,
    near, far, width, height, jitter); shadow: see BruteForceShadows.  Returns (value (H, W, 4), bound (H, W, 4), decided (H, W), info): |stored - value| <= bound is
    claimed for every decided pixel; info holds per-pixel facts about the rule's own evaluation (in shadow, lights drawn, candidates admitted, number of lights its mask lets through whose radius it lies beyond)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    h, w = instance_id.shape
    lit = instance_id >= 0
    py, px = np.nonzero(lit)
    n = len(px)
    ids = instance_id[lit]
    mat = {k: np.asarray([m[k] for m in materials], dtype=np.float64)[ids] for k in ("ignoreNormalFactor", "specularExponent", "shadowRayBias")}
    mask_bits = np.asarray([m["lightGroupMaskBits"] for m in materials], dtype=np.uint32)[ids]
    self_light = np.asarray([m["selfLight"] for m in materials], dtype=np.float64)[ids]
    rd = ray_direction(camera, normalised=(mutate == "raydir_normalised"))[lit]
    rd_err = CAM_K * U * np.abs(rd).max(axis=-1)
    st = {"position": vec(np.asarray(position, dtype=np.float64)[lit]), "normal": vec(np.asarray(normal, dtype=np.float64)[lit]),
          "specular": vec(np.asarray(specular, dtype=np.float64)[lit]), "rayDirection": [F(rd[:, c], rd_err) for c in range(3)],
          "px": px, "py": py, "bluenoise": bluenoise, "frameCount": int(frame_count), "diSamples": int(di_samples), "shadow": shadow,
          "ignoreNormalFactor": mat["ignoreNormalFactor"], "specularExponent": mat["specularExponent"], "shadowRayBias": mat["shadowRayBias"]}
    result, why, count, draws, outside, in_shadow = light_loop(st, mask_bits, lights, max_lights, mutate=mutate)

    result = [add(a, F(self_light[:, c])) for c, a in enumerate(result)]        # (D:51)
    normal, ray_dir, spec = st["normal"], st["rayDirection"], st["specular"]
    eye_lambert = fmax(dot3(normal, neg3(ray_dir)), 0.0)                        # (D:55), with the unnormalised direction
    eye_dot = dot3(reflect3(ray_dir, normal), neg3(ray_dir))
    if mutate != "eye_spec_unsaturated":
        eye_dot = saturate(eye_dot)                                             # (D:57)
    eye_spec = power(fmax(eye_dot, 0.0), st["specularExponent"])
    for c in range(3):
        eye = add(mul(float(eye_diffuse[c]), eye_lambert), mul(float(eye_specular[c]), mul(spec[c], eye_spec)))
        result[c] = add(result[c], eye)

    value = np.zeros((h, w, 4)); bound = np.zeros((h, w, 4))
    value[~lit] = (1.0, 1.0, 1.0, 0.0)
    v = np.stack([c.v for c in result], axis=-1); e = np.stack([c.e for c in result], axis=-1)
    value[lit] = np.concatenate([v, np.ones((n, 1))], axis=-1)
    # stored as f16: half a step of the value the device holds (at most |v| + e), never less than half a subnormal step
    b = e + np.maximum(F16_HALF_STEP * (np.abs(v) + e), F16_FLOOR)
    bound[lit] = np.concatenate([b, np.zeros((n, 1))], axis=-1)
    decided = np.ones((h, w), dtype=bool)
    why["bound"] = ~np.isfinite(b).all(axis=-1)                                 # no finite bound (an error interval that reaches a pole): not claimed either
    decided[lit] = ~(why["admission"] | why["walk"] | why["shadow"] | why["bound"])

    def full(x, fill=0):
        a = np.full((h, w), fill, dtype=x.dtype); a[lit] = x; return a
    info = {"in_shadow": full(in_shadow), "draws": full(draws), "candidates": full(count), "radii_outside": full(outside), "lit": lit,
            "undecided": {k: int(x.sum()) for k, x in why.items()}}
    return value, bound, decided, info
