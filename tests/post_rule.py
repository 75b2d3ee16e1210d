"""PostProcessPS as a rule in numpy float64 (rules X1-X8).  TEST INFRASTRUCTURE.

`post_process_kernel` (csrc/image_passes.hip) and `pass_post` / `sample_linear_wrap` (oracle/oracle_render.c) are the same lines twice; parity between them cannot
show a misreading that both share.  This module states the pass a third time, from PostProcessPS.hlsl (P:n), FullScreenVS.hlsl (V:n), the static sampler of
rt64_device.cpp:958-973 and the rectangles of rt64_view.cpp:1114-1136, 1258-1286, 1620-1626, in float64 on the error-carrying values of tests/light_rule.py.  It
imports nothing from oracle/ and was not written from the kernel.

Rules:

X1  Rectangles (rt64_view.cpp:1114-1136, 1258-1271).  The pass is drawn with the viewport and the scissor of the FIRST ray-traced instance.  An RT64_RECT
    (x, y, w, h) has its origin at the bottom-left of the screen: the scissor is [x, x + w) x [sh - y - h, sh - y), the viewport (x, sh - y - h, w, h), sh the screen's
    height.  A rectangle that is not set (w <= 0 or h <= 0: Instance::hasScissorRect / hasViewportRect) is the screen.
X2  Coverage (V:5-9, rt64_view.cpp:1624-1638).  The triangle covers the viewport; a back-buffer pixel (x, y) is written iff it lies inside the scissor -- left and top
    inclusive, right and bottom exclusive -- and its centre (x + 0.5, y + 0.5) inside the viewport.  There uv = (centre - viewport.xy) / viewport.wh: the interpolant
    runs from 0 to 1 across the VIEWPORT, not the screen.  The subtraction is exact (small integers and a half), the division is taken as 1 ulp.
X3  Outside (rt64_view.cpp:1292-1296, rt64_device.cpp:996-997).  A pixel the pass does not write keeps what the frame had there before: the back buffer cleared to
    (0, 0, 0, 255) with the background instances drawn over it.  gBackground (rt64_view.cpp:1298-1319, the BACKGROUND readback) is the same draw into a buffer cleared to
    (0, 0, 0, 0) without the instances' own rectangles; for background instances that are opaque (alpha 1: SRC_ALPHA / INV_SRC_ALPHA leaves the source) and carry no
    rectangles both draws store the same rgb, so the bytes are BACKGROUND's rgb with alpha 255.  The caller passes that image as `before`; without raster instances
    it is (0, 0, 0, 255) everywhere.
X4  Sampler (rt64_device.cpp:958-973: MIN_MAG_MIP_LINEAR, WRAP in u and v; SampleLevel 0).  texel = uv * size - 0.5 per axis (a texel's centre is at its index + 0.5);
    i = floor(texel), f = texel - i; the four texels (i, i + 1) x (j, j + 1), each index taken modulo the size (WRAP: -1 is the last texel, `size` the first);
    value = lerp(lerp(c00, c10, fx), lerp(c01, c11, fx), fy).  The filter is continuous in the coordinate, across texel boundaries and across the wrap: a coordinate
    known to +- e moves the value by at most e times the largest difference among the four taps (of either cell, where e reaches across a boundary), so the
    coordinate's roundings enter the BOUND and decide nothing.  The arithmetic of the three lerps adds its own roundings.
X5  Source.  gOutput is rtOutput at render size; behind an upscaler it is the upscaled image at screen size (rt64_view.cpp:800-801), and with
    upscalerSharpness > 0 this library's sharpened copy of it.  gFlow is always at render size.  The rule takes the source as a readback.
X6  Blur (P:14-31).  With motionBlurStrength > 0 and motionBlurSamples > 0: flow = sample(gFlow, uv).xy / resolution.xy (the RENDER size); where
    length(flow) > 1e-6f the colour is the mean of `samples` taps at clamp(uv - flow * strength / 2 + flow * s * (strength / samples), 0, 1), s = 0 .. samples - 1,
    summed in order and divided by the count.  A tap clamped to u = 1 has texel = size - 0.5: half the last column and, by WRAP, half the first; u = 0 likewise.
X7  The threshold (P:17) is the one decision.  length carries the bound of its own roundings (sampler, division, two products, a sum, a 1-ulp square root); where
    |length - 1e-6f| lies within it the pixel is held to the UNION of both branches' intervals and counted (`near_threshold`).
X8  Otherwise (P:34-35) the plain sample.  Alpha is 1: the byte 255.

The back buffer is UNORM8: a pixel inside the rectangles is held to [unorm8(value - bound), unorm8(value + bound)] per channel (compose_rule.to_final adds the
conversion's two roundings); a pixel outside them to `before`, byte for byte.  A pixel whose value or bound is not finite is NOT COVERED and counted; every case
requires the count to be 0.

Not covered: the upscaler's own stage (rules U1-U8 of oracle/oracle_upscale.c), the primary_spp mean, the HUD blend over the finished frame (tests/raster_rule.py),
debug views (DebugPS takes PostProcessPS's place), partitioned devices (they refuse a separate post pass)."""
import numpy as np

import compose_rule as CR
import light_rule as L
from light_rule import F, U, A

MUTATIONS = ("clamp_not_wrap", "no_half_texel", "taps_not_clamped", "start_not_halved", "flow_in_pixels", "step_over_samples_minus_one", "flow_nearest_at_screen_size",
             "rect_not_flipped", "scissor_inclusive", "uv_over_screen_not_viewport", "outside_left_black_over_background")

THRESHOLD = float(np.float32(1e-6))
CLEAR = (0, 0, 0, 255)


def _quot(a, b):
    """a / b, the division taken as 1 ulp; b exact and not 0."""
    v = a.v / b
    return F(v, a.e / abs(b) + A * np.abs(v))


def rectangles(screen, viewport, scissor, mutate=None):
    """(X1) -> viewport (x, y, w, h) and scissor (left, top, right, bottom) in back-buffer pixels, origin top-left."""
    sw, sh = screen
    vp, sc = (0, 0, sw, sh), (0, 0, sw, sh)
    top = (lambda y, h: y) if mutate == "rect_not_flipped" else (lambda y, h: sh - y - h)
    if viewport is not None and viewport[2] > 0 and viewport[3] > 0:
        x, y, w, h = (int(v) for v in viewport)
        vp = (x, top(y, h), w, h)
    if scissor is not None and scissor[2] > 0 and scissor[3] > 0:
        x, y, w, h = (int(v) for v in scissor)
        sc = (x, top(y, h), x + w, top(y, h) + h)
    return vp, sc


def coverage(screen, vp, sc, mutate=None):
    """(X2) -> inside (sh, sw) bool, u, v: F over the screen (meaningless outside)."""
    sw, sh = screen
    x, y = np.meshgrid(np.arange(sw, dtype=np.float64), np.arange(sh, dtype=np.float64), indexing="xy")
    cx, cy = x + 0.5, y + 0.5
    if mutate == "scissor_inclusive":
        inside = (x >= sc[0]) & (x <= sc[2]) & (y >= sc[1]) & (y <= sc[3])
    else:
        inside = (x >= sc[0]) & (x < sc[2]) & (y >= sc[1]) & (y < sc[3])
    inside &= (cx >= vp[0]) & (cx < vp[0] + vp[2]) & (cy >= vp[1]) & (cy < vp[1] + vp[3])
    if mutate == "uv_over_screen_not_viewport":
        u, v = _quot(F(cx), float(sw)), _quot(F(cy), float(sh))
    else:
        u, v = _quot(F(cx - vp[0]), float(vp[2])), _quot(F(cy - vp[1]), float(vp[3]))
    return inside, u, v


def _spread(img, ix, iy, address):
    """Largest difference among the four taps of the cell (ix, iy), per channel."""
    h, w = img.shape[:2]
    taps = np.stack([img[address(iy + dy, h), address(ix + dx, w)] for dy in (0, 1) for dx in (0, 1)], axis=0)
    return taps.max(axis=0) - taps.min(axis=0)


def sample(image, u, v, mutate=None):
    """(X4) image (H, W, C) at the coordinates u, v (F, any shape) -> (list of C values F, info: dict of bool arrays wrapped_left / right / top / bottom, edge_blend)."""
    img = np.asarray(image, dtype=np.float64)
    h, w = img.shape[:2]
    half = 0.0 if mutate == "no_half_texel" else 0.5
    tx, ty = L.sub(L.mul(u, float(w)), half), L.sub(L.mul(v, float(h)), half)
    ix, iy = np.floor(tx.v), np.floor(ty.v)
    fx, fy = tx.v - ix, ty.v - iy
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    if mutate == "clamp_not_wrap":
        address = lambda i, n: np.clip(i, 0, n - 1)
    else:
        address = lambda i, n: np.mod(i, n)
    x0, x1, y0, y1 = address(ix, w), address(ix + 1, w), address(iy, h), address(iy + 1, h)
    c00, c10, c01, c11 = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    # the coordinate's error (its own roundings and the one of texel - floor(texel), at most U) times the largest tap difference, over every cell the error reaches
    ex, ey = tx.e + U, ty.e + U
    spread = np.zeros_like(c00)
    for jx in (np.floor(tx.v - ex), np.floor(tx.v + ex)):
        for jy in (np.floor(ty.v - ey), np.floor(ty.v + ey)):
            spread = np.maximum(spread, _spread(img, jx.astype(np.int64), jy.astype(np.int64), address))
    out = []
    for c in range(img.shape[2]):
        top = L.add(F(c00[..., c]), L.mul(F(fx), L.sub(F(c10[..., c]), F(c00[..., c]))))
        bot = L.add(F(c01[..., c]), L.mul(F(fx), L.sub(F(c11[..., c]), F(c01[..., c]))))
        r = L.add(top, L.mul(F(fy), L.sub(bot, top)))
        out.append(F(r.v, r.e + (ex + ey) * spread[..., c]))
    info = dict(wrapped_left=ix < 0, wrapped_right=ix + 1 >= w, wrapped_top=iy < 0, wrapped_bottom=iy + 1 >= h,
                edge_blend=(fx == 0.5) & ((ix == -1) | (ix == w - 1)))
    return out, info


def post_process(source, flow, screen, render, strength, samples, viewport=None, scissor=None, before=None, mutate=None):
    """The rule for one frame.
    source (Hs, Ws, 4) float32: the image X5 names; flow (Hr, Wr, 2): FLOW; screen (sw, sh); render (rw, rh): resolution.xy; strength: motionBlurStrength; samples:
    motionBlurSamples; viewport, scissor: the first ray-traced instance's RT64_RECTs (x, y, w, h) or None; before (sh, sw, 4) uint8 or None: X3's buffer.
    Returns dict(value, bound (sh, sw, 3); lo, hi (sh, sw, 4) int64: the held interval (outside: `before`); inside, blurred, near_threshold, covered (sh, sw) bool;
    viewport, scissor; info: counts)."""
    sw, sh = int(screen[0]), int(screen[1])
    vp, sc = rectangles((sw, sh), viewport, scissor, mutate)
    inside, u, v = coverage((sw, sh), vp, sc, mutate)
    src = np.asarray(source, dtype=np.float64)[..., :3]
    plain, pinfo = sample(src, u, v, mutate)
    value = np.stack([c.v for c in plain], axis=-1); bound = np.stack([c.e for c in plain], axis=-1)
    blurred = np.zeros((sh, sw), dtype=bool); near = np.zeros((sh, sw), dtype=bool)
    flags = {k: pinfo[k] for k in ("wrapped_left", "wrapped_right", "wrapped_top", "wrapped_bottom")}
    extra = dict(clamped_left=np.zeros((sh, sw), dtype=bool), clamped_right=np.zeros((sh, sw), dtype=bool), clamped_top=np.zeros((sh, sw), dtype=bool),
                 clamped_bottom=np.zeros((sh, sw), dtype=bool), edge_blend=np.zeros((sh, sw), dtype=bool))
    lo, hi = CR.to_final(value, bound)
    strength = float(np.float32(strength)); samples = int(samples)
    if strength > 0.0 and samples > 0:
        fl = np.asarray(flow, dtype=np.float64)[..., :2]
        if mutate == "flow_nearest_at_screen_size":
            y, x = np.meshgrid(np.minimum(np.arange(sh), fl.shape[0] - 1), np.minimum(np.arange(sw), fl.shape[1] - 1), indexing="ij")
            f = [F(fl[y, x, 0]), F(fl[y, x, 1])]
        else:
            f, _ = sample(fl, u, v, mutate)
        if mutate != "flow_in_pixels":
            f = [_quot(f[0], float(render[0])), _quot(f[1], float(render[1]))]
        length = L.sqrt(L.add(L.mul(f[0], f[0]), L.mul(f[1], f[1])))
        blurred = length.v > THRESHOLD                                         # (X7)
        near = np.abs(length.v - THRESHOLD) <= length.e
        count = samples - 1 if mutate == "step_over_samples_minus_one" else samples
        q = float(np.float32(strength) / np.float32(max(count, 1)))
        step = F(q, A * abs(q))
        halved = (lambda a: a) if mutate == "start_not_halved" else (lambda a: F(a.v * 0.5, a.e * 0.5))          # / 2.0f is exact
        start = [L.sub(u, halved(L.mul(f[0], strength))), L.sub(v, halved(L.mul(f[1], strength)))]
        total = None
        bflags = {k: np.zeros((sh, sw), dtype=bool) for k in flags}
        for s in range(samples):
            uu = L.add(start[0], L.mul(L.mul(f[0], float(s)), step)); vv = L.add(start[1], L.mul(L.mul(f[1], float(s)), step))
            extra["clamped_left"] |= uu.v < 0.0; extra["clamped_right"] |= uu.v > 1.0; extra["clamped_top"] |= vv.v < 0.0; extra["clamped_bottom"] |= vv.v > 1.0
            if mutate != "taps_not_clamped":
                uu, vv = L.saturate(uu), L.saturate(vv)
            c, info = sample(src, uu, vv, mutate)
            for k in bflags:
                bflags[k] |= info[k]
            extra["edge_blend"] |= info["edge_blend"]
            total = c if total is None else [L.add(a, b) for a, b in zip(total, c)]
        mean = [_quot(t, float(samples)) for t in total]
        bv = np.stack([c.v for c in mean], axis=-1); be = np.stack([c.e for c in mean], axis=-1)
        blo, bhi = CR.to_final(bv, be)
        plo, phi = lo, hi
        m = blurred[..., None]
        value, bound = np.where(m, bv, value), np.where(m, be, bound)
        lo, hi = np.where(m, blo, plo), np.where(m, bhi, phi)
        n = near[..., None]
        lo, hi = np.where(n, np.minimum(blo, plo), lo), np.where(n, np.maximum(bhi, phi), hi)
        for k in flags:
            flags[k] = np.where(blurred, bflags[k], flags[k])
        for k in extra:
            extra[k] &= blurred
    covered = np.isfinite(value).all(axis=-1) & np.isfinite(bound).all(axis=-1)
    if before is None:
        before = np.broadcast_to(np.array(CLEAR, dtype=np.uint8), (sh, sw, 4))
    alpha = np.full((sh, sw, 1), 255, dtype=np.int64)
    before = np.concatenate([np.asarray(before).astype(np.int64)[..., :3], alpha], axis=-1)          # (X3) its rgb, alpha 255
    if mutate == "outside_left_black_over_background":
        before[:, :sc[0], :3] = 0
    lo4 = np.where(inside[..., None], np.concatenate([lo, alpha], axis=-1), before)
    hi4 = np.where(inside[..., None], np.concatenate([hi, alpha], axis=-1), before)
    x, y = np.meshgrid(np.arange(sw), np.arange(sh), indexing="xy")
    counts = {k: int((inside & m).sum()) for k, m in list(flags.items()) + list(extra.items())}
    counts.update(clamped_taps=int((inside & (extra["clamped_left"] | extra["clamped_right"] | extra["clamped_top"] | extra["clamped_bottom"])).sum()),
                  near_threshold=int((inside & near).sum()), blurred=int((inside & blurred).sum()), inside=int(inside.sum()), outside_rectangle=int((~inside).sum()),
                  outside_left=int((~inside & (x < max(vp[0], sc[0]))).sum()), outside_right=int((~inside & (x >= min(vp[0] + vp[2], sc[2]))).sum()),
                  outside_top=int((~inside & (y < max(vp[1], sc[1]))).sum()), outside_bottom=int((~inside & (y >= min(vp[1] + vp[3], sc[3]))).sum()),
                  two_candidates=int((inside & (hi > lo).any(axis=-1)).sum()), not_covered=int((inside & ~covered).sum()))
    return dict(value=value, bound=bound, lo=lo4, hi=hi4, inside=inside, blurred=blurred, near_threshold=near, covered=covered, viewport=vp, scissor=sc,
                info=dict(counts=counts))


def compare(final, rule):
    """FINAL_RGBA8 against the rule.  Returns dict(bad: pixels inside the rectangles outside their interval or not covered; outside_bad: pixels outside them that differ
    from `before`; ratio: (largest, mean) over the inside pixels of the distance between the rule's value and the colours that convert to the stored byte, over the
    bound: under 1 exactly where the byte lies in the interval)."""
    f = np.asarray(final).astype(np.int64)
    off = ((f < rule["lo"]) | (f > rule["hi"])).any(axis=-1)
    inside = rule["inside"]
    bound = rule["bound"] + U * (2.0 * np.clip(np.abs(rule["value"]), 0.0, 1.0) + 0.5 / 255.0)
    c = f[..., :3].astype(np.float64)
    below, above = (c - 0.5) / 255.0, (c + 0.5) / 255.0                     # the colours that convert to the byte; 0 and 255 take everything past them
    below = np.where(c == 0, -np.inf, below); above = np.where(c == 255, np.inf, above)
    dist = np.maximum(np.maximum(below - rule["value"], rule["value"] - above), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dist == 0.0, 0.0, dist / bound)
    r = np.where(np.isnan(r), np.inf, r).max(axis=-1)
    if rule["near_threshold"].any():                                        # held to the union of two intervals: the ratio to one value says nothing there
        r = np.where(rule["near_threshold"] & ~off, 0.0, r)
    sel = r[inside]
    return dict(bad=int((inside & (off | ~rule["covered"])).sum()), outside_bad=int((~inside & off).sum()),
                ratio=(float(sel.max()) if sel.size else 0.0, float(np.where(np.isfinite(sel), sel, 1e9).mean()) if sel.size else 0.0),
                where=inside & off)
