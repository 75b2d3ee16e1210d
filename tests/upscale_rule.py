"""The temporal upscaler as a rule in numpy (rules U1-U8).  TEST INFRASTRUCTURE.

`taa_upsample_kernel` (csrc/upscale.hip) and `oupscale_frame` (oracle/oracle_upscale.c) are the same lines twice, written side by side from one comment; parity between
them cannot show a misreading that both share, and a whole-image RMSE cannot show a fault on a few hundred pixels.  This module states U1-U8 a third time, from their
meaning, vectorised over the display pixels.  It imports nothing from oracle/.

Two kinds of quantity:

DECISIONS are exact IEEE float32 operations on the device and on the host (+ - x /, floor, comparisons; the build has -ffp-contract=off and IEEE division), and DESIGN.md
fixes their order.  The rule evaluates them in numpy float32 in that order and holds a pixel to the float32 result:
    U1 / U2  u = (x + 0.5) / dw;  r = u * rw;  i0 = clamp(floor(r - j.x), 0, rw - 1)                      (y likewise)
    U4       the smallest depth of the nine taps, the first one on ties (rows, then columns): comparisons of stored float32 values
    U5       uvPrev = u + flow.x / rw;  0 <= uvPrev <= 1;  floor(uvPrev * dw - 0.5);  N > 0 (N: the bilinear count, float32 in the kernel's order)
Each is evaluated in float64 too.  Where the two disagree the pixel is counted (`on_grid_x`, `on_grid_y`, `range_edge`, `cell_edge`) and held to the float32 decision;
`near_grid_x`, `near_grid_y` count the pixels whose float64 r - j lies within its own error of an integer, the ones for which the float32 order matters at all.  A
disagreement further from the edge than the float64 value's first-order error is not a rounding: the pixel is NOT DECIDED.  No decision needs two candidates.

VALUES are float64 on the error-carrying `F` of tests/light_rule.py: the distances, the Gaussian weights (exp2: 1 ulp), the weighted mean (an IEEE division: half an ulp),
the colour box (exact), the bilinear history -- its cell is the float32 decision, its fraction the float64 position minus that cell, so a `cell_edge` pixel has a fraction
just outside [0, 1) and the position's error times the taps' differences is in the bound: the filter is continuous across the choice --, the clamp, the lock lerp, the
blend factor, the output and the count channel.  Every float32 operation is half an ulp, carried first order.

The mask readbacks are the float32 `(float)byte / 255.0f` of the stored UNORM8, the expression the kernel applies to the byte (device_math.h from_unorm8 on both
paths): the rule takes them as exact.  FLOW readbacks are exact float16 values.
"""
import hashlib

import numpy as np

import light_rule as L
from light_rule import F, U, A

MUTATIONS = ("jitter_subtracted", "floor_without_jitter", "distance_from_clamped_index", "sigma_two", "flow_of_centre", "flow_of_farthest", "tie_takes_last",
             "flow_in_display_pixels", "flow_subtracted", "masks_of_nearest_depth", "history_nearest", "history_no_half_texel", "off_screen_clamped_not_dropped",
             "no_colour_clamp", "lock_ignored", "lock_inverted", "reactive_ignored", "conf_dropped", "one_over_n", "cap_64", "history_is_sharpened")

f32 = np.float32
K_WIDTH = float(f32(2.88539008))          # 2 / ln 2: w = exp(-2 d^2)
CONF_SCALE = float(f32(0.1))
CAP = 32.0
UPSCALER_AUTO, UPSCALER_FSR = 1, 3
MODE_AUTO, MODE_ULTRA_PERFORMANCE, MODE_PERFORMANCE, MODE_BALANCED, MODE_QUALITY, MODE_ULTRA_QUALITY, MODE_NATIVE = range(7)
COUNTS = ("taps_clamped_left", "taps_clamped_right", "taps_clamped_top", "taps_clamped_bottom", "i0_clamped", "k0_clamped", "flow_not_centre", "depth_tie",
          "history_off_screen", "history_clamped_edge", "outside_box", "locked_outside_box", "reactive_wins", "conf_wins", "count_wins", "capped", "fresh",
          "on_grid_x", "on_grid_y", "near_grid_x", "near_grid_y", "range_edge", "cell_edge")


# ---- the frame's jitter and sizes (restated; tests/test_upscale_rule.py holds both against the oracle) ------------------------------------------------

def halton(i, b):
    """HaltonSequence in float32 (the restatement of tests/test_upscaler.py)."""
    f, r = f32(1.0), f32(0.0)
    while i > 0:
        f = f32(f / f32(b)); r = f32(r + f * f32(i % b)); i //= b
    return r


def jitter(frame_index, phases):
    """The jitter of the frame_index-th frame a view draws (from 0), as the two float32 the kernel receives."""
    i = frame_index % phases + 1
    return float(f32(halton(i, 2) - f32(0.5))), float(f32(halton(i, 3) - f32(0.5)))


def quality(mode, dw, dh):
    """(render width, render height, jitter phases) of a quality mode at a display size."""
    if mode == MODE_AUTO:
        px = dw * dh
        mode = (MODE_ULTRA_QUALITY if px <= 1280 * 720 else MODE_QUALITY if px <= 1920 * 1080 else MODE_BALANCED if px <= 2560 * 1440 else
                MODE_PERFORMANCE if px <= 3840 * 2160 else MODE_ULTRA_PERFORMANCE)
    if mode == MODE_NATIVE:
        w, h = dw, dh
    elif mode == MODE_ULTRA_QUALITY:
        w, h = dw * 77 // 100, dh * 77 // 100
    else:
        ratio = f32({MODE_QUALITY: 1.5, MODE_BALANCED: 1.7, MODE_PERFORMANCE: 2.0, MODE_ULTRA_PERFORMANCE: 3.0}[mode])
        w, h = int(f32(dw) / ratio), int(f32(dh) / ratio)
    w, h = max(w, 1), max(h, 1)
    q = f32(dw) / f32(w)
    return w, h, max(int(f32(8.0) * f32(q * q)), 1)


# ---- small things on F --------------------------------------------------------------------------------------------------------------------------------

def _quot(a, b):
    """a / b as an IEEE division: half an ulp.  b: F or exact, away from 0 by more than its error."""
    b = b if isinstance(b, F) else F(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = a.v / b.v
        lo = np.abs(b.v) - b.e
        e = np.where(lo > 0.0, (a.e + np.abs(v) * b.e) / np.where(lo > 0.0, lo, 1.0), np.inf) + U * np.abs(v)
    return F(v, e)


def _exp2_neg(a):
    """exp2(-a), the device's exp2 taken as 1 ulp (tests/light_rule.py A)."""
    v = np.exp2(-a.v)
    return F(v, v * np.expm1(np.log(2.0) * a.e) + A * v)


def _clamp(a, lo, hi):
    """fmin(fmax(a, lo), hi) with exact ends: the clamped ends of v +- e."""
    v = np.clip(a.v, lo, hi)
    return F(v, np.maximum(np.clip(a.v + a.e, lo, hi) - v, v - np.clip(a.v - a.e, lo, hi)))


def _max(a, b):
    return F(np.maximum(a.v, b.v), np.maximum(a.e, b.e))


def _row(a):
    return F(a.v[None, :], a.e[None, :])


def _col(a):
    return F(a.v[:, None], a.e[:, None])


def _axis(n_display, n_render, j, mutate):
    """U1 / U2 along one axis.  Returns dict(u32, u: F, r: F, i0 (clamped, the float32 decision), raw (unclamped), on_grid, near, decided)."""
    x = np.arange(n_display)
    u32 = (x.astype(f32) + f32(0.5)) / f32(n_display)
    r32 = u32 * f32(n_render)
    jf = f32(0.0) if mutate == "floor_without_jitter" else f32(j)
    raw = np.floor(r32 - jf).astype(np.int64)
    u = _quot(F(x + 0.5), float(n_display))
    r = L.mul(u, float(n_render))
    t = L.sub(r, float(jf))
    raw64 = np.floor(t.v).astype(np.int64)
    near = np.abs(t.v - np.round(t.v)) <= t.e
    return dict(u32=u32, u=u, r=r, raw=raw, i0=np.clip(raw, 0, n_render - 1), on_grid=raw != raw64, near=near, decided=(raw == raw64) | near)


def upsample(color, flow, reactive, lock, depth, jitter, prev, display_size, mutate=None):
    """The rule for one frame.
    color (rh, rw, 4) float32: OUTPUT_RGBA32F; flow (rh, rw, 2): FLOW; reactive, lock, depth (rh, rw); jitter (j.x, j.y): the frame's, from `jitter`; prev (dh, dw, 4)
    float32: the previous frame's UPSCALED, or None without a history; display_size (dw, dh).
    Returns dict(value, bound (dh, dw, 3); count, count_bound (dh, dw); count_exact, fresh, decided, covered (dh, dw) bool; info: dict(counts))."""
    assert mutate is None or mutate in MUTATIONS, mutate
    color = np.asarray(color, dtype=np.float32); depth = np.asarray(depth, dtype=np.float32)
    flow = np.asarray(flow, dtype=np.float32); reactive = np.asarray(reactive, dtype=np.float32); lock = np.asarray(lock, dtype=np.float32)
    rh, rw = color.shape[:2]
    dw, dh = int(display_size[0]), int(display_size[1])
    assert flow.shape == (rh, rw, 2) and reactive.shape == lock.shape == depth.shape == (rh, rw)
    jx, jy = float(f32(jitter[0])), float(f32(jitter[1]))
    if mutate == "jitter_subtracted":
        jx, jy = -jx, -jy
    ax, ay = _axis(dw, rw, jx, mutate), _axis(dh, rh, jy, mutate)
    I0 = np.broadcast_to(ax["i0"][None, :], (dh, dw)); K0 = np.broadcast_to(ay["i0"][:, None], (dh, dw))

    # U3: the nine taps, rows then columns
    K = float(f32(1.44269504)) if mutate == "sigma_two" else K_WIDTH
    c64 = color.astype(np.float64)
    sumw, sums = F(np.zeros((dh, dw))), [F(np.zeros((dh, dw))) for _ in range(3)]
    cmin, cmax = np.full((dh, dw, 3), np.inf), np.full((dh, dw, 3), -np.inf)
    best = np.full((dh, dw), -np.inf if mutate == "flow_of_farthest" else np.inf, dtype=np.float32)
    bi, bk = I0.copy(), K0.copy()
    seen = []
    conf = None
    for dk in (-1, 0, 1):
        k = ay["i0"] + dk
        kc = np.clip(k, 0, rh - 1)
        sy = L.add(F((kc if mutate == "distance_from_clamped_index" else k) + 0.5), jy)
        dy = L.sub(ay["r"], sy)
        dy2 = _col(L.mul(dy, dy))
        for di in (-1, 0, 1):
            i = ax["i0"] + di
            ic = np.clip(i, 0, rw - 1)
            sx = L.add(F((ic if mutate == "distance_from_clamped_index" else i) + 0.5), jx)
            dx = L.sub(ax["r"], sx)
            w = _exp2_neg(L.mul(L.add(_row(L.mul(dx, dx)), dy2), K))
            KC, IC = np.broadcast_to(kc[:, None], (dh, dw)), np.broadcast_to(ic[None, :], (dh, dw))
            c = c64[KC, IC]
            sumw = L.add(sumw, w)
            for ch in range(3):
                sums[ch] = L.add(sums[ch], L.mul(w, F(c[..., ch])))
            cmin = np.minimum(cmin, c[..., :3]); cmax = np.maximum(cmax, c[..., :3])
            if di == 0 and dk == 0:
                conf = w
            z = depth[KC, IC]                                                             # U4
            take = z > best if mutate == "flow_of_farthest" else (z <= best if mutate == "tie_takes_last" else z < best)
            best = np.where(take, z, best); bi = np.where(take, IC, bi); bk = np.where(take, KC, bk)
            seen.append((z, IC, KC))
    ties = sum((z == best) & ((IC != bi) | (KC != bk)) for z, IC, KC in seen)          # another render pixel with the chosen depth
    if mutate == "flow_of_centre":
        bi, bk = I0, K0
    cur = [_quot(s, sumw) for s in sums]
    fx32, fy32 = flow[bk, bi, 0], flow[bk, bi, 1]
    mi, mk = (bi, bk) if mutate == "masks_of_nearest_depth" else (I0, K0)
    reac = np.clip(reactive[mk, mi].astype(np.float64), 0.0, 1.0); lk = np.clip(lock[mk, mi].astype(np.float64), 0.0, 1.0)
    if mutate == "lock_ignored":
        lk = np.zeros_like(lk)
    if mutate == "lock_inverted":
        lk = 1.0 - lk
    if mutate == "reactive_ignored":
        reac = np.zeros_like(reac)

    # U5: the history
    sign = f32(-1.0) if mutate == "flow_subtracted" else f32(1.0)
    over_x, over_y = (dw, dh) if mutate == "flow_in_display_pixels" else (rw, rh)
    pu32 = ax["u32"][None, :] + sign * fx32 / f32(over_x); pv32 = ay["u32"][:, None] + sign * fy32 / f32(over_y)
    pu = L.add(_row(ax["u"]), _quot(F(float(sign) * fx32.astype(np.float64)), float(over_x)))
    pv = L.add(_col(ay["u"]), _quot(F(float(sign) * fy32.astype(np.float64)), float(over_y)))
    have = prev is not None
    inside32 = (pu32 >= 0) & (pu32 <= 1) & (pv32 >= 0) & (pv32 <= 1)
    inside64 = (pu.v >= 0) & (pu.v <= 1) & (pv.v >= 0) & (pv.v <= 1)
    at_edge = (np.minimum(np.abs(pu.v), np.abs(pu.v - 1.0)) <= pu.e) | (np.minimum(np.abs(pv.v), np.abs(pv.v - 1.0)) <= pv.e)
    range_edge = inside32 != inside64
    decided = np.broadcast_to(ax["decided"][None, :] & ay["decided"][:, None], (dh, dw)) & (~range_edge | at_edge)
    if mutate == "off_screen_clamped_not_dropped":
        pu32, pv32 = np.clip(pu32, f32(0), f32(1)), np.clip(pv32, f32(0), f32(1))
        pu, pv = _clamp(pu, 0.0, 1.0), _clamp(pv, 0.0, 1.0)
        inside32 = np.ones((dh, dw), dtype=bool)
    fetched = inside32 & have
    zero = F(np.zeros((dh, dw)))
    h = [zero, zero, zero]; N = zero
    positive = np.zeros((dh, dw), dtype=bool)
    cell_edge = np.zeros((dh, dw), dtype=bool); clamped_edge = np.zeros((dh, dw), dtype=bool)
    if have:
        p32 = np.asarray(prev, dtype=np.float32)
        assert p32.shape == (dh, dw, 4)
        if mutate == "history_is_sharpened":
            import sharpen_rule
            p32 = sharpen_rule.rcas_f32(p32, 1.0)[0]
        p64 = p32.astype(np.float64)
        half = 0.0 if mutate == "history_no_half_texel" else 0.5
        hx32 = pu32 * f32(dw) - f32(half); hy32 = pv32 * f32(dh) - f32(half)
        hx = L.sub(L.mul(pu, float(dw)), half); hy = L.sub(L.mul(pv, float(dh)), half)
        if mutate == "history_nearest":
            hx32, hy32 = np.floor(hx32 + f32(0.5)), np.floor(hy32 + f32(0.5))
            hx, hy = F(hx32.astype(np.float64)), F(hy32.astype(np.float64))
        x0f, y0f = np.floor(hx32), np.floor(hy32)
        for pos, cell in ((hx, x0f), (hy, y0f)):
            differs = (np.floor(pos.v) != cell) & fetched
            cell_edge |= differs
            decided = decided & (~differs | (np.abs(pos.v - np.round(pos.v)) <= pos.e))
        tx32, ty32 = hx32 - x0f, hy32 - y0f
        tx, ty = F(hx.v - x0f, hx.e), F(hy.v - y0f, hy.e)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        clamped_edge = fetched & ((x0 < 0) | (x0 + 1 > dw - 1) | (y0 < 0) | (y0 + 1 > dh - 1))
        xa, xb, ya, yb = np.clip(x0, 0, dw - 1), np.clip(x0 + 1, 0, dw - 1), np.clip(y0, 0, dh - 1), np.clip(y0 + 1, 0, dh - 1)

        def bilinear(ch):
            c00, c10, c01, c11 = F(p64[ya, xa, ch]), F(p64[ya, xb, ch]), F(p64[yb, xa, ch]), F(p64[yb, xb, ch])
            top = L.add(c00, L.mul(tx, L.sub(c10, c00))); bot = L.add(c01, L.mul(tx, L.sub(c11, c01)))
            return L.add(top, L.mul(ty, L.sub(bot, top)))
        h = [L.where(fetched, bilinear(ch), zero) for ch in range(3)]
        N = L.where(fetched, bilinear(3), zero)
        # N > 0 in float32, in the kernel's order
        c00, c10, c01, c11 = p32[ya, xa, 3], p32[ya, xb, 3], p32[yb, xa, 3], p32[yb, xb, 3]
        top32 = c00 + tx32 * (c10 - c00); bot32 = c01 + tx32 * (c11 - c01)
        n32 = top32 + ty32 * (bot32 - top32)
        positive = fetched & (n32 > 0)
        decided = decided & (~fetched | ((N.v > 0) == (n32 > 0)) | (np.abs(N.v) <= N.e))

    # U6, U7
    w_count = _quot(F(np.ones((dh, dw))), L.sub(N, 0.0) if mutate == "one_over_n" else L.add(N, 1.0))
    w_conf = L.mul(conf, CONF_SCALE)
    a = w_count if mutate == "conf_dropped" else _max(w_count, w_conf)
    a = _max(a, F(reac))
    a = L.where(positive, a, F(np.ones((dh, dw))))
    top_term = np.maximum(np.maximum(w_count.v, w_conf.v), reac)
    value, bound = np.empty((dh, dw, 3)), np.empty((dh, dw, 3))
    outside = np.zeros((dh, dw), dtype=bool)
    for ch in range(3):
        hc = h[ch] if mutate == "no_colour_clamp" else _clamp(h[ch], cmin[..., ch], cmax[..., ch])
        outside |= (h[ch].v < cmin[..., ch]) | (h[ch].v > cmax[..., ch])
        hc = L.add(hc, L.mul(F(lk), L.sub(h[ch], hc)))
        out = L.add(hc, L.mul(a, L.sub(cur[ch], hc)))
        value[..., ch], bound[..., ch] = out.v, out.e
    cap = 64.0 if mutate == "cap_64" else CAP
    count = _clamp(L.add(N, 1.0), -np.inf, cap)
    surely_capped = (N.v + 1.0) * (1.0 - U) - N.e >= cap
    count_exact = ~fetched | surely_capped                       # no history: N is 0 and the count 1; N + 1 past the cap by more than its error: the cap
    count_bound = np.where(count_exact, 0.0, count.e)
    covered = np.isfinite(value).all(axis=-1) & np.isfinite(bound).all(axis=-1) & np.isfinite(count.v) & np.isfinite(count_bound)

    tie = ties > 0
    masks = dict(
        taps_clamped_left=I0 == 0, taps_clamped_right=I0 == rw - 1, taps_clamped_top=K0 == 0, taps_clamped_bottom=K0 == rh - 1,
        i0_clamped=np.broadcast_to((ax["raw"] != ax["i0"])[None, :], (dh, dw)), k0_clamped=np.broadcast_to((ay["raw"] != ay["i0"])[:, None], (dh, dw)),
        flow_not_centre=(bi != I0) | (bk != K0), depth_tie=tie, history_off_screen=~inside32 & have, history_clamped_edge=clamped_edge,
        outside_box=positive & outside, locked_outside_box=positive & outside & (lk > 0.0),
        reactive_wins=positive & (reac >= top_term) & (reac > 0.0), conf_wins=positive & (w_conf.v >= top_term) & (reac < top_term),
        count_wins=positive & (w_count.v >= top_term) & (w_conf.v < top_term) & (reac < top_term), capped=count.v == cap, fresh=~positive,
        on_grid_x=np.broadcast_to(ax["on_grid"][None, :], (dh, dw)), on_grid_y=np.broadcast_to(ay["on_grid"][:, None], (dh, dw)),
        near_grid_x=np.broadcast_to(ax["near"][None, :], (dh, dw)), near_grid_y=np.broadcast_to(ay["near"][:, None], (dh, dw)), range_edge=range_edge & have, cell_edge=cell_edge)
    counts = {k: int(masks[k].sum()) for k in COUNTS}
    counts["not_decided"] = int((~decided).sum()); counts["not_covered"] = int((~covered).sum()); counts["pixels"] = dh * dw
    return dict(value=value, bound=bound, count=count.v, count_bound=count_bound, count_exact=count_exact, fresh=~positive, decided=decided, covered=covered,
                masks=masks, info=dict(counts=counts, render=(rw, rh), display=(dw, dh)))


def compare(upscaled, rule):
    """UPSCALED against the rule.  Returns dict(ratio (dh, dw): the largest |stored - value| / bound over rgb; count_dev (dh, dw): |stored.a - count|; bad: the pixels
    with ratio >= 1, or undecided, or uncovered; count_bad: the pixels whose count channel is outside its bound (exact where the rule says so); largest, mean)."""
    up = np.asarray(upscaled, dtype=np.float64)
    assert up.shape[:2] == rule["value"].shape[:2] and up.shape[2] == 4, up.shape
    diff = np.abs(up[..., :3] - rule["value"])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0.0, 0.0, diff / rule["bound"])
    r = np.where(np.isnan(r), np.inf, r).max(axis=-1)
    dev = np.abs(up[..., 3] - rule["count"])
    dev = np.where(np.isnan(dev), np.inf, dev)
    bad = (r >= 1.0) | ~rule["decided"] | ~rule["covered"]
    count_bad = dev > rule["count_bound"]
    return dict(ratio=r, count_dev=dev, bad=bad, count_bad=count_bad, largest=float(r.max()), mean=float(np.where(np.isfinite(r), r, 1e9).mean()))


def key(*arrays):
    """A digest of input bytes: a rule result is cached under it."""
    h = hashlib.sha1()
    for a in arrays:
        if a is None:
            h.update(b"none"); continue
        a = np.ascontiguousarray(a)
        h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()
