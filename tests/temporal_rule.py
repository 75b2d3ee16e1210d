"""Temporal accumulation of the GI pass as a rule in numpy float64 (rules N1-N8).  TEST INFRASTRUCTURE.

`history_weight` and the accumulation around the sample loop (`indirect_kernel` and `bounce_resolve_kernel` in csrc/passes.hip) and their C restatement in
oracle/oracle_render.c (`history_weight`, `pass_indirect`) were written from the same HLSL.  This module states the step a third time, from its meaning, in float64,
on top of the error-carrying values of tests/light_rule.py (`F`: value and a first-order bound on what float32 arithmetic and 1-ulp exp2 / log2 / rcp may do to
it).  It imports nothing from oracle/.

The fresh sample of a frame is never stored, only its blend with the history.  The rule therefore takes the fresh radiance from a TWIN session B that draws the
same calls as the session A under test, but whose compared frame N has denoiserEnabled = 0: giReproject = 0 and nothing else the bounce reads changes (same
frameCount, G-buffer, rays).  B's INDIRECT_LIGHT_RAW at N is the fresh radiance (the sample rounded to float16 for giSamples = 1, the running mean for n > 1, alpha
n); B's GI_MOMENTS are the fresh (sum L / n, sum L^2 / n) in float32 exactly, because lerp(0, x, 1) = 0 + (x - 0) * 1 = x.  The rule predicts A's frame N from A's
frame N - 1 (INDIRECT_LIGHT_RAW, GI_MOMENTS, DEPTH, SHADING_NORMAL), A's frame N (FLOW, DEPTH, SHADING_NORMAL, INSTANCE_ID) and B's fresh images.  It never reads
A's INDIRECT_LIGHT_RAW or GI_MOMENTS at N.

Rules (I:n = IndirectRayGen.hlsl line n):

N1  Previous pixel (I:43-44).  j = (trunc(x + 0.5 + flow.x), trunc(y + 0.5 + flow.y)) with the flow as stored (float16): the cast truncates toward zero, so a sum
    in (-1, 0) lands on column / row 0, inside the image.  Outside [0, W) x [0, H) every previous value (depth, normal, colour, history, moments) is 0.  The
    float32 sum (x + 0.5f) + flow cannot change the truncation: x + 0.5 is exact; a flow of magnitude >= 1/2 is a multiple of 2^-11 and the sum, below 2^12, is
    exact in 24 bits; a flow of magnitude < 1/2 leaves the sum strictly inside (x, x + 1), rounding is monotone and the integers are float32 values, so the sum
    can at most round ONTO x or x + 1 - 2^-12 <= ... < x + 1, never past an integer.  The rule checks |flow| < 2^11 and that a float32 evaluation gives the same
    pixel; a pixel is undecided only if that check fails.
N2  History weight (I:46-56).  w = exp(-|depth - prevDepth| / 0.01f) * pow(max(0, prevNormal . normal), 128).  No clamp at 1: float16 normals have lengths off 1
    and the weight exceeds 1 where both are long.  pow of 0 is 0.  Bound: the subtraction and the division round once each (the division is taken as 1 ulp);
    exp(-t) is taken as exp2(-t * log2 e): the constant and the product round once each, which is a relative 2 U t on the result, and exp2 is 1 ulp (libm's
    expf, which the oracle calls, is inside this); pow is exp2(128 * log2 x) with log2's absolute error near 1 as light_rule.LOG_FLOOR.  A weight below
    2^-150 is exactly 0 in float32; a weight that is not may be flushed while it, or a factor, is subnormal: 2^-125 is added to its bound.
N3  History length (I:56, 126).  h0 = prev.a * w, then per sample h = min(h + 1, 64) and c = c + (r - c) / h, starting from c = prev.rgb.
N4  Stored values (I:131).  rgb = float16(c), alpha = float16(h).  Bound: half a float16 step at the value plus the propagated terms.  For giSamples = 1 the
    fresh sample r is known as B's float16: its half step enters divided by h.
N5  Several samples.  With h_k = h0 + k (the cap does not bind while h0 + n <= 64), c_k = c_(k-1) + (r_k - c_(k-1)) / h_k gives
    c_k h_k = c_(k-1) (h_k - 1) + r_k = c_(k-1) h_(k-1) + r_k, hence by induction c_n h_n = prev h0 + sum r_k:
        c = (prev * h0 + n * mean) / (h0 + n),   mean = sum r_k / n,
    and B's stored rgb is that mean (the same recurrence from h0 = 0).  The n steps round a few times each on magnitudes up to |prev| + n mean (radiances are not
    negative, so r_k <= n mean): ROUND_K U n (|prev| + n mean) is added.  Where the cap can bind inside the loop (h0 + n > 64 within h0's bound) the samples are
    not separable: the pixel is NOT COVERED (neither held nor undecided).  With n = 1 every pixel is covered.
N6  Moments (I:126-131 extended by SVGF's luminance moments).  m = prevM[j] + (fresh - prevM[j]) * min(n / h, 1) with h the float32 history BEFORE its float16
    rounding and `fresh` B's GI_MOMENTS; prevM is 0 out of range.  Bound: the roundings of the division, the subtraction, the product and the sum, and h's error.
N7  No surface (INSTANCE_ID < 0), or giSamples = 0: rgb = float16(ambientBase + ambientNoGI) (one float32 sum), alpha 0, moments (0, 0), all exact.
N8  What the twin must satisfy, checked by the rule's caller on every run (temporal_cases.hold): A's and B's frame N - 1 images are equal byte for byte; B's alpha
    is giSamples on surfaces and 0 elsewhere; where this rule's h0 is exactly 0, h is 1 and both lerps have t = 1: a + (b - a) * 1 in float32, which is b bit for
    bit where a is 0.  So A's moments are that expression of the previous moments and B's, evaluated in float32, bit for bit wherever h0 = 0, and A's rgb and moments
    are B's bit for bit wherever the previous pixel lies off the frame.  (Behind a previous pixel INSIDE the frame with h0 = 0 -- a cosine <= 0 at a silhouette -- the
    colour's b is known only as float16 and a + (b - a) may round: such a pixel is held by N4's bound, one float16 step, and no tighter.)

Not covered: samples under a binding cap with n > 1 (N5); frames whose mirrors rewrite SHADING_NORMAL (the guide normal[prev] is then not the readback);
primary_spp > 1; interleaved strips."""
import numpy as np

import light_rule as L
from light_rule import F, U, A

MUTATIONS = ("floor_not_trunc", "no_half_pixel", "flow_subtracted", "previous_at_current_pixel", "edge_clamped_not_zero", "depth_scale_tenth", "normal_exponent_64",
             "weight_clamped_at_one", "history_unweighted", "cap_before_increment", "no_cap", "moments_at_current_pixel", "moments_alpha_one", "alpha_not_history",
             "guides_of_current_frame")

CAP = 64.0
DEPTH_SCALE = float(np.float32(0.01))
FLOW_LIMIT = 2.0 ** 11
ZERO_BELOW = 2.0 ** -150          # half the smallest float32 subnormal: anything under it is 0
FLUSH = 2.0 ** -126               # the smallest normal float32: a subnormal result may be flushed to 0
ROUND_K = 8                       # float32 roundings of one step of the sample loop (N5), an upper estimate


def f16_half_step(v):
    """Half the distance between neighbouring float16 values around |v| (the subnormal step below 2^-14)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0.0, a, 1.0)))
    e = np.where(a > 0.0, np.maximum(e, -14.0), -14.0)
    return 2.0 ** (e - 11.0)


def stored_f16(x):
    """A float32 quantity within x.v +- x.e, stored as float16: the value and the bound of the stored number.  A quantity without an error of its own (a history of
    exactly 1 or 64) is stored as its float16, exactly."""
    exact = x.e == 0.0
    with np.errstate(over="ignore"):
        rounded = x.v.astype(np.float16).astype(np.float64)
    return np.where(exact, rounded, x.v), np.where(exact, 0.0, x.e + f16_half_step(np.abs(x.v) + x.e))


def fmin(a, c):
    m = L.fmax(L.neg(a), -c)
    return F(-m.v, m.e)


def previous_pixel(flow, mutate=None):
    """(N1) -> (jx, jy, inside, decided), each (H, W)."""
    flow = np.asarray(flow)
    h, w = flow.shape[:2]
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="xy")
    fx, fy = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    ok = np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < FLOW_LIMIT) & (np.abs(fy) < FLOW_LIMIT)
    fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
    if mutate == "flow_subtracted":
        fx, fy = -fx, -fy
    half = 0.0 if mutate == "no_half_pixel" else 0.5
    cast = np.floor if mutate == "floor_not_trunc" else np.trunc
    jx, jy = cast(x + half + fx), cast(y + half + fy)
    # the float32 evaluation, left to right, must land on the same pixel
    sx = (x.astype(np.float32) + np.float32(half)) + fx.astype(np.float32); sy = (y.astype(np.float32) + np.float32(half)) + fy.astype(np.float32)
    ok &= (cast(sx.astype(np.float64)) == jx) & (cast(sy.astype(np.float64)) == jy)
    if mutate == "previous_at_current_pixel":
        jx, jy = x, y
    inside = (jx >= 0) & (jy >= 0) & (jx < w) & (jy < h)
    if mutate == "edge_clamped_not_zero":
        jx, jy = np.clip(jx, 0, w - 1), np.clip(jy, 0, h - 1)
        inside = np.ones_like(inside)
    return np.where(inside, jx, 0).astype(np.int64), np.where(inside, jy, 0).astype(np.int64), inside, ok


def _fetch(image, jx, jy, inside):
    """Load at the previous pixel; 0 outside the image."""
    v = np.asarray(image, dtype=np.float64)[jy, jx]
    return np.where(inside if v.ndim == 2 else inside[..., None], v, 0.0)


def history_weight(depth, normal, prev_depth, prev_normal, mutate=None):
    """(N2) on values already fetched: depth, prev_depth (H, W); normal, prev_normal (H, W, 3+).  Returns F."""
    d = L.sub(F(depth), F(prev_depth))
    t = L.mul(F(np.abs(d.v), d.e), F(1.0 / (float(np.float32(0.1)) if mutate == "depth_scale_tenth" else DEPTH_SCALE)))
    t = F(t.v, t.e + A * t.v)                                                  # the division: 1 ulp
    ev = np.exp(-t.v)
    # exp(-t) as exp2(-t * log2 e): the constant and the product round once each, 2 U t log2 e on the argument, times ln 2 on the result; t's own error goes through
    # whole; exp2 is 1 ulp, counted twice so that libm's expf (the oracle's) lies inside as well
    we = F(ev, ev * (t.e + 2.0 * U * t.v + 2.0 * A))
    cosine = L.fmax(L.dot3(L.vec(np.asarray(prev_normal, dtype=np.float64)), L.vec(np.asarray(normal, dtype=np.float64))), 0.0)
    wn = L.power(cosine, 64.0 if mutate == "normal_exponent_64" else 128.0)
    wn = F(np.where(cosine.v == 0.0, 0.0, wn.v), np.where((cosine.v == 0.0) & (cosine.e == 0.0), 0.0, wn.e))      # pow(0, 128) = 0
    w = L.mul(we, wn)
    zero = w.v + w.e < ZERO_BELOW
    w = F(np.where(zero, 0.0, w.v), np.where(zero, 0.0, w.e + 2.0 * FLUSH))          # a factor, or the product, flushed while subnormal (the other factor is under 2)
    if mutate == "weight_clamped_at_one":
        w = fmin(w, 1.0)
    return w


def accumulate(cur, prev, fresh, samples, ambient, mutate=None):
    """The rule for one frame.
    cur: dict(flow (H, W, 2), depth (H, W), normal (H, W, 4), id (H, W)) of frame N;  prev: dict(raw (H, W, 4), moments (H, W, 2), depth, normal) of frame N - 1;
    fresh: dict(raw, moments) of the twin at frame N;  samples: giSamples;  ambient: (ambientBase, ambientNoGI), two rgb triples.
    Returns dict(value, bound (H, W, 4): INDIRECT_LIGHT_RAW; moments, moments_bound (H, W, 2); decided, covered, surface, zero_history (H, W) bool; weight, h0,
    history: F; prev_x, prev_y, inside; info)."""
    n = int(samples)
    ident = np.asarray(cur["id"])
    surface = (ident >= 0) & (n > 0)
    jx, jy, inside, decided = previous_pixel(cur["flow"], mutate)
    depth = np.asarray(cur["depth"], dtype=np.float64); normal = np.asarray(cur["normal"], dtype=np.float64)[..., :3]
    guides = cur if mutate == "guides_of_current_frame" else prev
    w = history_weight(depth, normal, _fetch(guides["depth"], jx, jy, inside), _fetch(np.asarray(guides["normal"])[..., :3], jx, jy, inside), mutate)
    acc = _fetch(prev["raw"], jx, jy, inside)
    if mutate == "moments_at_current_pixel":
        prev_m = np.asarray(prev["moments"], dtype=np.float64)
    else:
        prev_m = _fetch(prev["moments"], jx, jy, inside)
    h0 = F(acc[..., 3]) if mutate == "history_unweighted" else L.mul(F(acc[..., 3]), w)
    zero_history = (h0.v == 0.0) & (h0.e == 0.0)
    fresh_raw = np.asarray(fresh["raw"], dtype=np.float64); fresh_m = np.asarray(fresh["moments"], dtype=np.float64)
    covered = np.ones(ident.shape, dtype=bool)
    value = np.zeros(ident.shape + (4,)); bound = np.zeros_like(value)
    if n <= 1:
        if mutate == "cap_before_increment":
            h = L.add(fmin(h0, CAP), 1.0)
        elif mutate == "no_cap":
            h = L.add(h0, 1.0)
        else:
            h = fmin(L.add(h0, 1.0), CAP)
        h = F(h.v, np.where(zero_history, 0.0, h.e))                         # 0 + 1 does not round
        inv = L.rcp(h)
        for k in range(3):
            r = F(fresh_raw[..., k], f16_half_step(fresh_raw[..., k]))       # (N4) the sample behind B's float16
            c = L.add(F(acc[..., k]), L.mul(L.sub(r, F(acc[..., k])), inv))  # lerp(c, r, 1 / h)
            value[..., k], bound[..., k] = stored_f16(c)
    else:
        # (N5) (prev * h0 + n * mean) / (h0 + n) where the cap cannot bind
        covered = h0.v + h0.e + n <= CAP                                     # (the wrong variants of the cap agree with the rule here)
        h = L.add(h0, float(n))
        h = F(h.v, np.where(zero_history, 0.0, h.e))                         # 0 + 1 + ... + 1 does not round
        inv = L.rcp(h)
        for k in range(3):
            mean = F(fresh_raw[..., k], f16_half_step(fresh_raw[..., k]) + ROUND_K * U * n * n * np.abs(fresh_raw[..., k]))
            c = L.mul(L.add(L.mul(F(acc[..., k]), h0), L.mul(mean, float(n))), inv)
            c = F(c.v, c.e + ROUND_K * U * n * (np.abs(acc[..., k]) + n * np.abs(fresh_raw[..., k])))
            value[..., k], bound[..., k] = stored_f16(c)
    if mutate == "alpha_not_history":
        value[..., 3], bound[..., 3] = float(n), 0.0
    else:
        value[..., 3], bound[..., 3] = stored_f16(h)
    # (N6)
    alpha_m = F(np.ones_like(h.v)) if mutate == "moments_alpha_one" else fmin(L.mul(F(float(n)), L.rcp(h)), 1.0)
    moments = np.zeros(ident.shape + (2,)); moments_bound = np.zeros_like(moments)
    for k in range(2):
        m = L.add(F(prev_m[..., k]), L.mul(L.sub(F(fresh_m[..., k]), F(prev_m[..., k])), alpha_m))
        moments[..., k], moments_bound[..., k] = m.v, m.e
    # (N7)
    base, no_gi = (np.asarray(a, dtype=np.float32) for a in ambient)
    sky = (base + no_gi).astype(np.float16).astype(np.float64)
    value[~surface, :3], value[~surface, 3] = sky, 0.0
    bound[~surface] = 0.0; moments[~surface] = 0.0; moments_bound[~surface] = 0.0
    decided = np.where(surface, decided, True)
    covered = np.where(surface, covered, True)
    x, y = np.meshgrid(np.arange(ident.shape[1], dtype=np.float64), np.arange(ident.shape[0], dtype=np.float64), indexing="xy")
    flow = np.asarray(cur["flow"], dtype=np.float64)
    sx, sy = x + 0.5 + flow[..., 0], y + 0.5 + flow[..., 1]
    counts = dict(
        truncation_x=int((surface & (sx > -1.0) & (sx < 0.0)).sum()), truncation_y=int((surface & (sy > -1.0) & (sy < 0.0)).sum()),
        off_left=int((surface & (sx <= -1.0)).sum()), off_right=int((surface & (sx >= ident.shape[1])).sum()),
        off_top=int((surface & (sy <= -1.0)).sum()), off_bottom=int((surface & (sy >= ident.shape[0])).sum()),
        above_one=int((surface & (w.v > 1.0)).sum()), below_one=int((surface & (w.v < 1.0) & (w.v > 0.95)).sum()),
        intermediate=int((surface & (w.v > 0.05) & (w.v < 0.95)).sum()), disoccluded=int((surface & inside & (w.v < 1e-3)).sum()),
        zero_history=int((surface & zero_history).sum()), capped=int((surface & (h.v >= CAP) & (n <= 1)).sum()),
        capped_before=int((surface & (acc[..., 3] >= CAP)).sum()), fixed_point=int((surface & (h.v < CAP) & (h.v > 32.0)).sum()),
        flow_y=int((surface & (flow[..., 1] != 0.0)).sum()), grown=int((surface & (h.v > acc[..., 3] + 1.0) & (h.v < CAP)).sum()))
    return dict(value=value, bound=bound, moments=moments, moments_bound=moments_bound, decided=decided, covered=covered, surface=surface, zero_history=surface & zero_history,
                weight=w, h0=h0, history=h, prev_x=jx, prev_y=jy, inside=inside, info=dict(counts=counts))


def _ratio(stored, value, bound):
    dev = np.abs(np.asarray(stored, dtype=np.float64) - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dev == 0.0, 0.0, dev / bound)
    return np.where(np.isnan(r), np.inf, r)


def compare(raw, moments, rule):
    """Stored INDIRECT_LIGHT_RAW and GI_MOMENTS of A's frame N against the rule, over the decided and covered pixels.
    Returns ({"rgb" | "alpha" | "moments": (largest ratio, mean ratio)}, bad (H, W) bool)."""
    held = rule["decided"] & rule["covered"]
    r_raw = _ratio(np.asarray(raw)[..., :4], rule["value"], rule["bound"])
    r_m = _ratio(moments, rule["moments"], rule["moments_bound"])
    parts = {"rgb": r_raw[..., :3].max(axis=-1), "alpha": r_raw[..., 3], "moments": r_m.max(axis=-1)}
    bad = np.zeros(held.shape, dtype=bool)
    out = {}
    for k, r in parts.items():
        bad |= held & ~(r < 1.0)
        sel = r[held]
        out[k] = (float(sel.max()) if sel.size else 0.0, float(np.where(np.isfinite(sel), sel, 1e9).mean()) if sel.size else 0.0)
    return out, bad
