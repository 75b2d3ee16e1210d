"""The raster (HUD / background) pass of one frame as a rule in numpy float64 (rules Z1-Z10).  TEST INFRASTRUCTURE.

csrc/raster.hip + csrc/raster_pixel.h and oracle/oracle_raster.c are one algorithm (raster spec S0-S8: a Sutherland-Hodgman clipper, a fan, 24.8 snapping,
integer edge functions) written twice by one hand.  This module states the same operation a third time from the meaning of the pipeline and has NO clipper, no fan and
no snapping: a pixel is covered where the homogeneous edge functions of the clip-space triangle, its depth, its w and the guard band say so at the pixel's centre
(Z2), an attribute is the clip-space barycentric mix of the three vertices' values (Z5), a layer is blended into the bytes the layer before it stored (Z8).  It imports
nothing from oracle/ and nothing from the library; the texture term is tests/sampler_rule.py's, the combiner tests/material_rule.py's formula functions, the arithmetic
the `F` value-and-bound arithmetic of tests/light_rule.py.

Every condition of Z2 is linear in the pixel position and has a signed distance to its zero line in pixels.  A pixel is decided *outside* a triangle when one condition
fails by more than DELTA, *inside* when all hold by more than DELTA, and undecided otherwise; a pixel with an undecided layer is undecided (Z3).  Where the three vertices
of a triangle land on exact 24.8 coordinates and nothing is clipped, coverage is evaluated in integers with the top-left rule, and no pixel is undecided (Z4).

The result per pixel and channel is the interval of bytes a correct float32 implementation may store (Z9), or "undecided".
"""
import numpy as np

import light_rule as L
import material_rule as M
import sampler_rule as T
from light_rule import F, U

DELTA = 1.0 / 64.0         # px.  24.8 snapping moves a vertex by at most 2^-9 px per axis, the float32 evaluation of a clipped vertex inside the guard band by about 2^-11 px
                           # at these frame sizes; 1/64 is four times the sum.  Not tuned: a side that needs more has something to explain.
SNAP_PX = 2.0 ** -8        # what a vertex may move by (2^-9 sqrt 2 + 2^-11, rounded up): an attribute moves by its screen gradient times this
W_EPS = 2.0 ** -20         # a point is in front of the eye when w > 2^-20
GUARD = 4.0                # the guard band, in NDC units: the project's choice (Z2)
# Upper estimate of the float32 roundings between the vertices' values and an attribute at a pixel: edge value and area to float (2), three quotients (1 each on a
# path), 1 / w and its product (2), three products and two sums (3 on a path), the sum of the weights (2), the quotient (1): 11; a clipped piece's corner values add
# the parameter of each cut (3), its lerp (3) for up to three planes and the mix of the original values (5): 23 more.  Taken as 48, in the manner of CAM_K / SHADOW_K.
ATTR_K = 48
BLEND_K = 8                # byte / 255 (2), two products, 1 - a, the sum (4): 6, taken as 8
FILTER_EPS = M.FILTER_EPS

MUTATIONS = ("bottom_right_rule", "pixel_corner", "affine_attributes", "rw_not_reoriented", "y_not_flipped", "rect_origin_top_left", "scissor_right_inclusive",
             "back_faces_culled", "near_plane_ignored", "far_plane_ignored", "guard_band_at_one", "clipped_attributes_from_piece_corners", "no_byte_round_trip",
             "premultiplied_blend", "draw_order_reversed", "background_after_foreground", "gradients_zero")

COUNTS = ("covered", "two_layers", "ties", "back_facing", "clipped", "cut_near", "cut_far", "cut_guard", "behind_one", "behind_two", "scissored", "minified", "magnified",
          "exact_triangles", "drawn_triangles", "empty_triangles")


def rect_pixels(rect, h, top_left=False):
    """(Z1) An RT64_RECT (x, y, w, h), origin bottom-left, y up -> (left, top, right, bottom) on the pixel grid, origin top-left, y down; right and bottom exclusive."""
    x, y, rw, rh = (int(v) for v in rect)
    top = y if top_left else h - y - rh
    return x, top, x + rw, top + rh


def to_byte(x):
    return np.clip(np.floor(np.asarray(x, dtype=np.float64) * 255.0 + 0.5), 0, 255).astype(np.int64)


def _representable(v):
    v = np.asarray(v, dtype=np.float64)
    return bool((v.astype(np.float32).astype(np.float64) == v).all())


def _exact_vertices(P, vp):
    """(Z4) The three vertices as exact 24.8 integers (X [3], Y [3]) when the triangle needs no clipping and every step of x / w -> NDC -> pixels is exact in float32
    (so that no implementation can land elsewhere); None otherwise."""
    x, y, z, w = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    if not ((w > W_EPS).all() and (z >= 0).all() and (z <= w).all() and (np.abs(x) <= GUARD * w).all() and (np.abs(y) <= GUARD * w).all()):
        return None
    m, e = np.frexp(w)
    if not (m == 0.5).all():                                       # w a power of two: the division is exact however it is done
        return None
    vx, vy, vw, vh = vp
    steps = [x / w, y / w, (x / w) * 0.5 + 0.5, 0.5 - (y / w) * 0.5, ((x / w) * 0.5 + 0.5) * vw, (0.5 - (y / w) * 0.5) * vh]
    X = (((x / w) * 0.5 + 0.5) * vw + vx) * 256.0; Y = ((0.5 - (y / w) * 0.5) * vh + vy) * 256.0
    if not all(_representable(s) for s in steps) or not (X == np.round(X)).all() or not (Y == np.round(Y)).all() or max(np.abs(X).max(), np.abs(Y).max()) >= 2.0 ** 22:
        return None
    return X.astype(np.int64), Y.astype(np.int64)


def _polygon(P):
    """Only for the wrong variant `clipped_attributes_from_piece_corners`: the visible polygon of a triangle, clip-space corners (n, 4) in float64."""
    planes = [lambda v: v[3] - W_EPS, lambda v: v[2], lambda v: v[3] - v[2], lambda v: v[0] + GUARD * v[3], lambda v: GUARD * v[3] - v[0],
              lambda v: v[1] + GUARD * v[3], lambda v: GUARD * v[3] - v[1]]
    poly = [P[k].copy() for k in range(3)]
    for d in planes:
        out = []
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            da, db = d(a), d(b)
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                out.append(a + (da / (da - db)) * (b - a))
        poly = out
        if len(poly) < 3:
            return []
    return poly


class _Lines:
    """(Z2) The homogeneous edge functions of a clip-space triangle (3, 4) over a grid of pixel positions: c[k] >= 0 inside, sum(c w) = |D|."""

    def __init__(self, P, vp, sx, sy, flip_y=True):
        xyw = P[:, [0, 1, 3]]
        self.D = float(np.linalg.det(xyw))
        s = 1.0 if self.D >= 0 else -1.0
        self.lines = np.stack([np.cross(xyw[(k + 1) % 3], xyw[(k + 2) % 3]) for k in range(3)]) * s      # [k] . (xn, yn, 1)
        self.vp, self.flip = vp, flip_y
        self.sx, self.sy = sx, sy

    def ndc(self, sx, sy):
        vx, vy, vw, vh = self.vp
        xn = (sx - vx) / vw * 2.0 - 1.0
        yn = 1.0 - (sy - vy) / vh * 2.0 if self.flip else (sy - vy) / vh * 2.0 - 1.0
        return xn, yn

    def c(self, sx, sy):
        xn, yn = self.ndc(sx, sy)
        return [self.lines[k, 0] * xn + self.lines[k, 1] * yn + self.lines[k, 2] for k in range(3)]

    def distance(self, f):
        """Signed distance in pixels of every pixel to the zero line of sum_k c_k f_k (positive where it holds); +inf where it holds identically."""
        f = np.asarray(f, dtype=np.float64)
        if (f == 0.0).all():
            return np.full(self.sx.shape, np.inf)
        g = f @ self.lines
        xn, yn = self.ndc(self.sx, self.sy)
        val = g[0] * xn + g[1] * yn + g[2]
        grad = np.hypot(g[0] * 2.0 / self.vp[2], g[1] * 2.0 / self.vp[3])
        if grad > 0.0:
            return val / grad
        return np.where(val == 0.0, 0.0, np.sign(val) * np.inf)                            # the same everywhere: its sign decides


def _weights(c, w=None):
    """Clip-space barycentrics from the edge functions; with w, the screen-space (affine) ones."""
    if w is not None:
        c = [c[k] * w[k] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = c[0] + c[1] + c[2]
        return [ck / s for ck in c]


def _mix(l, a):
    return l[0] * a[0] + l[1] * a[1] + l[2] * a[2]


def draw(target, instances, width, height, rows=None, apply_rects=True, mutate=None, state=None):
    """One draw list over `target` ((H, W, 4) uint8: the bytes before the list).  instances: dicts in draw order with
         pos (N, 4) clip-space positions, indices (3 T), inputs [(N, 4)] the combiner's vertex inputs (alpha 1 without the alpha option), uv (N, 2) or None,
         shader_id, filter, haddr, vaddr, levels (list of (h, w, 4) uint8, level 0 first) or None, viewport / scissor (RT64_RECT or None).
    rows: (H,) bool, the rows this device owns (band and strips); None = all.  apply_rects False: the list is drawn without viewports and scissors (gBackground).
    state: the result of the list drawn before this one over the same target (its intervals and undecided pixels carry on).
    Returns dict(lo, hi (H, W, 4) int64 byte intervals, flo, fhi (H, W, 4) the last layer's float interval, undecided (H, W) bool, layers (H, W) decided covering
    layers, counts)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    H, W = height, width
    if state is None:
        t = np.asarray(target, dtype=np.int64)
        state = dict(lo=t.copy(), hi=t.copy(), flo=t / 255.0, fhi=t / 255.0, undecided=np.zeros((H, W), dtype=bool), layers=np.zeros((H, W), dtype=np.int64),
                     counts={k: 0 for k in COUNTS}, edge_hits=np.zeros((H, W), dtype=np.int64))
    st = state
    cnt = st["counts"]
    own = np.ones(H, dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
    py, px = np.mgrid[0:H, 0:W]
    off = 0.0 if mutate == "pixel_corner" else 0.5
    sx, sy = px + off, py + off
    work = []
    for inst in instances:
        idx = np.asarray(inst["indices"], dtype=np.int64).reshape(-1, 3)
        work += [(inst, tri) for tri in idx]
    if mutate == "draw_order_reversed":
        work = work[::-1]
    for inst, tri in work:
        top_left = mutate == "rect_origin_top_left"
        vp = (0.0, 0.0, float(W), float(H)); sc = (0, 0, W, H)
        if apply_rects:                                                                   # (Z1) a rect with no area is "not set"
            if inst.get("scissor") and inst["scissor"][2] > 0 and inst["scissor"][3] > 0:
                sc = rect_pixels(inst["scissor"], H, top_left)
            if inst.get("viewport") and inst["viewport"][2] > 0 and inst["viewport"][3] > 0:
                l, t_, r, b = rect_pixels(inst["viewport"], H, top_left)
                vp = (float(l), float(t_), float(r - l), float(b - t_))
        right = sc[2] + (1 if mutate == "scissor_right_inclusive" else 0)
        allowed = (px >= sc[0]) & (px < right) & (py >= sc[1]) & (py < sc[3]) & own[:, None]
        P = np.asarray(inst["pos"], dtype=np.float64)[tri]
        ln = _Lines(P, vp, sx, sy, flip_y=mutate != "y_not_flipped")
        if ln.D == 0.0 or (mutate == "back_faces_culled" and ln.D < 0.0) or (P[:, 3] <= 0).all():
            cnt["empty_triangles"] += 1
            continue
        w, z = P[:, 3], P[:, 2]
        needs_clip = not ((w > W_EPS).all() and (z >= 0).all() and (z <= w).all() and (np.abs(P[:, 0]) <= GUARD * w).all() and (np.abs(P[:, 1]) <= GUARD * w).all())
        exact = _exact_vertices(P, vp) if mutate not in ("y_not_flipped",) else None
        # ---- coverage ----------------------------------------------------------------------------------------------------------------------
        if exact is not None:                                                             # (Z4)
            X, Y = exact
            cx = (256 * px + int(256 * off)).astype(np.int64); cy = (256 * py + int(256 * off)).astype(np.int64)
            inside = np.ones((H, W), dtype=bool); tie = np.zeros((H, W), dtype=bool)
            area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
            if area == 0:
                cnt["empty_triangles"] += 1
                continue
            for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                sgn = 1 if ((X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])) > 0 else -1
                e = ((X[b] - X[a]) * (cy - Y[a]) - (Y[b] - Y[a]) * (cx - X[a])) * sgn      # > 0 on the side of the third vertex
                dedx, dedy = -(Y[b] - Y[a]) * sgn, (X[b] - X[a]) * sgn
                # a centre ON the edge belongs to the triangle when the edge is a left edge (the inside lies at larger x) or a top edge (horizontal, the inside below)
                keeps = (dedx > 0 or (dedx == 0 and dedy > 0)) if mutate != "bottom_right_rule" else (dedx < 0 or (dedx == 0 and dedy < 0))
                inside &= (e > 0) | ((e == 0) & keeps)
                tie |= e == 0
                closed = (e >= 0) if a == 0 else closed & (e >= 0)
            tie &= closed                                                                  # a centre on an edge or a vertex of the triangle itself
            und = np.zeros((H, W), dtype=bool)
            cnt["exact_triangles"] += 1
            cnt["ties"] += int((tie & allowed).sum())
            st["edge_hits"] += (tie & allowed)
            why = {}
        else:                                                                             # (Z2), (Z3)
            d_edges = np.minimum(np.minimum(ln.distance([1, 0, 0]), ln.distance([0, 1, 0])), ln.distance([0, 0, 1]))
            d_w = ln.distance(w / W_EPS - 1.0)
            d_near = ln.distance(z) if mutate != "near_plane_ignored" else np.full((H, W), np.inf)
            d_far = ln.distance(w - z) if mutate != "far_plane_ignored" else np.full((H, W), np.inf)
            g = 1.0 if mutate == "guard_band_at_one" else GUARD
            xn, yn = ln.ndc(sx, sy)
            d_guard = np.minimum((g - np.abs(xn)) * vp[2] / 2.0, (g - np.abs(yn)) * vp[3] / 2.0)
            m = np.minimum(np.minimum(np.minimum(d_edges, d_w), np.minimum(d_near, d_far)), d_guard)
            inside = m > DELTA
            und = ~inside & ~(m < -DELTA)
            why = dict(cut_near=(d_edges > DELTA) & (d_near < -DELTA), cut_far=(d_edges > DELTA) & (d_far < -DELTA),
                       cut_guard=(d_edges > DELTA) & (d_w > DELTA) & (d_guard < -DELTA))
        cnt["scissored"] += int(((inside | und) & ~allowed).sum())
        inside &= allowed; und &= allowed
        for k, v in why.items():
            cnt[k] += int((v & allowed).sum())
        st["undecided"] |= und
        sel = inside & ~st["undecided"]
        if not sel.any():
            cnt["empty_triangles"] += int(not und.any())
            continue
        cnt["drawn_triangles"] += 1
        n_behind = int((w <= 0).sum())
        cnt["back_facing"] += int(sel.sum()) if ln.D < 0 else 0
        cnt["clipped"] += int(sel.sum()) if needs_clip else 0
        cnt["behind_one"] += int(sel.sum()) if n_behind == 1 else 0
        cnt["behind_two"] += int(sel.sum()) if n_behind == 2 else 0
        # ---- attributes (Z5) ----------------------------------------------------------------------------------------------------------------
        qx, qy = sx[sel], sy[sel]
        n = len(qx)

        def weights_at(ax, ay):
            c = ln.c(ax, ay)
            if mutate == "affine_attributes":
                return _weights(c, w)
            if mutate == "rw_not_reoriented" and ln.D < 0:
                ws = w[[0, 2, 1]]                                                          # the weights of screen space divided by the w of the wrong corners
                return _weights([c[k] * w[k] / ws[k] for k in range(3)])
            return _weights(c)
        l0, lx, ly = weights_at(qx, qy), weights_at(qx + 1.0, qy), weights_at(qx, qy + 1.0)
        piece = None
        if mutate == "clipped_attributes_from_piece_corners" and needs_clip:
            poly = _polygon(P)
            piece = []
            for j in range(1, len(poly) - 1):
                pl = _Lines(np.stack([poly[0], poly[j], poly[j + 1]]), vp, sx, sy)
                piece.append(pl)

        def attribute(values):
            """values (3,) of the three vertices -> F at the pixels, and the values one pixel right and one pixel down on the triangle's plane."""
            a = np.asarray(values, dtype=np.float64)
            v, vx, vy = _mix(l0, a), _mix(lx, a), _mix(ly, a)
            if piece:
                for pl in piece:                                                           # the piece's own barycentrics on the ORIGINAL vertices' values
                    c = pl.c(qx, qy)
                    inp = (c[0] >= 0) & (c[1] >= 0) & (c[2] >= 0)
                    v = np.where(inp, _mix(_weights(c), a), v)
            e = ATTR_K * U * np.abs(a).max() + SNAP_PX * np.hypot(vx - v, vy - v)
            return F(v, e), vx, vy
        one, zero = F(np.ones(n)), F(np.zeros(n))
        cc = M._combiner(inst["shader_id"])
        inputs = []
        for i in range(4):
            if i < cc["inputs"]:
                raw = np.asarray(inst["inputs"][i], dtype=np.float64)[tri]
                val = [attribute(raw[:, ch])[0] for ch in range(4 if cc["alpha"] else 3)]
                inputs.append(val if cc["alpha"] else val + [one])
            else:
                inputs.append([zero, zero, zero, zero])
        t0 = [zero, zero, zero, zero]
        if cc["tex0"] and inst.get("levels"):                                              # (Z6)
            lv = inst["levels"]
            h0, w0 = lv[0].shape[:2]
            uv = np.asarray(inst["uv"], dtype=np.float64)[tri]
            (u, ux, uy), (v, vx_, vy_) = attribute(uv[:, 0]), attribute(uv[:, 1])
            ddx = np.stack([ux - u.v, vx_ - v.v], axis=1); ddy = np.stack([uy - u.v, vy_ - v.v], axis=1)
            if mutate == "gradients_zero":
                ddx = np.zeros_like(ddx); ddy = np.zeros_like(ddy)
            raw_lod, rho = T.raw_lod(ddx, ddy, w0, h0)
            drho = 2.0 * np.sqrt(2.0) * np.maximum(u.e * w0, v.e * h0)
            with np.errstate(divide="ignore", invalid="ignore"):
                dlod = np.where(rho > 0.0, np.minimum(drho / (np.where(rho > 0.0, rho, 1.0) * np.log(2.0)) + U * np.abs(np.where(np.isfinite(raw_lod), raw_lod, 0.0)) + L.LOG_FLOOR, len(lv)), 0.0)
            du = u.e + 2.0 * U * np.abs(u.v); dv = v.e + 2.0 * U * np.abs(v.v)
            r = T.sample_grad_bounds(lv, u.v, v.v, ddx, ddy, inst["filter"], inst["haddr"], inst["vaddr"], du, dv, dlod, FILTER_EPS)
            t0 = [F(0.5 * (r["vmin"][:, c] + r["vmax"][:, c]), 0.5 * (r["vmax"][:, c] - r["vmin"][:, c]) + FILTER_EPS) for c in range(4)]
            cnt["minified"] += int((r["lod"] >= 1.0).sum()); cnt["magnified"] += int((rho < 1.0).sum())
        t1 = [one, zero, one, one]
        if not cc["same"] and cc["alpha"]:                                                # (Z7) the combiner: separate colour and alpha formulas
            src = M._color_formula(cc, False, True, inputs, t0, t1, one, zero)
            src[3] = M._alpha_formula(cc, inputs, t0, t1, zero)
        else:
            src = M._color_formula(cc, cc["alpha"], cc["alpha"], inputs, t0, t1, one, zero)
        src = [L.saturate(L._f(s)) for s in src]
        # ---- blend (Z8) ---------------------------------------------------------------------------------------------------------------------
        a = src[3]
        ia_lo, ia_hi = np.clip(1.0 - a.v - a.e - U, 0.0, 1.0), np.clip(1.0 - a.v + a.e + U, 0.0, 1.0)
        if mutate == "no_byte_round_trip":
            dlo, dhi = st["flo"][sel], st["fhi"][sel]
        else:
            dlo, dhi = st["lo"][sel] / 255.0, st["hi"][sel] / 255.0
        flo = np.empty((n, 4)); fhi = np.empty((n, 4))
        for ch in range(4):
            s = a if ch == 3 else (src[ch] if mutate == "premultiplied_blend" else L.mul(src[ch], a))
            flo[:, ch] = (s.v - s.e) + dlo[:, ch] * ia_lo - BLEND_K * U
            fhi[:, ch] = (s.v + s.e) + dhi[:, ch] * ia_hi + BLEND_K * U
        st["flo"][sel], st["fhi"][sel] = np.clip(flo, 0.0, 1.0), np.clip(fhi, 0.0, 1.0)
        st["lo"][sel], st["hi"][sel] = to_byte(flo), to_byte(fhi)
        st["layers"][sel] += 1
    cnt["covered"] = int(((st["layers"] > 0) & ~st["undecided"]).sum())
    cnt["two_layers"] = int(((st["layers"] >= 2) & ~st["undecided"]).sum())
    return st


def frame(scene, mutate=None):
    """(Z10) The pass of one frame.  scene: dict(width, height, instances (scene order, each with `background`: bool), rows (or None), base: None for a frame with
    no ray-traced instance (the buffer cleared to `clear`; the background list is drawn into it first), else the (H, W, 4) uint8 of OUTPUT_RGBA32F the foreground list lies over).
    gBackground is cleared to 0 and drawn without viewports and scissors.  Returns dict(final, background): results of `draw`; background is None without a
    background instance."""
    W, H = scene["width"], scene["height"]
    bg = [i for i in scene["instances"] if i["background"]]
    fg = [i for i in scene["instances"] if not i["background"]]
    zero = np.zeros((H, W, 4), dtype=np.uint8)
    cleared = np.broadcast_to(np.asarray(scene.get("clear", (0, 0, 0, 0)), dtype=np.uint8), (H, W, 4))
    m = None if mutate == "background_after_foreground" else mutate
    background = draw(zero, bg, W, H, rows=None, apply_rects=False, mutate=m) if bg else None
    if scene.get("base") is None:
        lists = (fg, bg) if mutate == "background_after_foreground" else (bg, fg)
        final = draw(cleared, lists[0], W, H, rows=scene.get("rows"), mutate=m)
        final = draw(None, lists[1], W, H, rows=scene.get("rows"), mutate=m, state=final)
    else:
        final = draw(scene["base"], fg, W, H, rows=scene.get("rows"), mutate=m)
    return dict(final=final, background=background)


def judge(result, image, rows=None):
    """A stored RGBA8 image against a `draw` result.  Returns dict(wrong: decided pixels with a byte outside its interval, undecided, share_max, share_mean: the
    used share of the colour bound over the channels of the decided pixels exactly one layer covers, bad (H, W) bool)."""
    img = np.asarray(image).astype(np.int64)
    mine = np.ones(img.shape[:2], dtype=bool) if rows is None else np.broadcast_to(np.asarray(rows, dtype=bool)[:, None], img.shape[:2])
    dec = ~result["undecided"] & mine
    out = ((img < result["lo"]) | (img > result["hi"])).any(axis=-1)
    bad = dec & out
    # the stored byte b stands for the values (b +- 0.5) / 255: what the centre of the rule's interval must move by to reach them, over half the interval's width
    mid = 0.5 * (result["flo"] + result["fhi"]) * 255.0; half = 0.5 * (result["fhi"] - result["flo"]) * 255.0
    dev = np.maximum(np.abs(img - mid) - 0.5, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(dev == 0.0, 0.0, dev / half).max(axis=-1)
    m = dec & (result["layers"] == 1)              # one layer: the bound of the arithmetic alone; under more layers the interval also spans the bytes the lower layer may have stored
    return dict(wrong=int(bad.sum()), undecided=int((result["undecided"] & mine).sum()),
                share_max=float(share[m].max()) if m.any() else 0.0, share_mean=float(share[m].mean()) if m.any() else 0.0, bad=bad)
