"""Material records of ray-query hits as a rule in numpy float64 (rules H1-H10).  TEST INFRASTRUCTURE.

`hit_material_kernel` (csrc/material.hip) makes its records with the device functions the frame's any-hit programs run (csrc/shade.h).  This module states
the same operation from its meaning: the hit's triangle in the mesh as the host sent it, barycentric interpolation of UV and colour inputs (tests/surface_rule.py
for the fetch, the interpolation and A7's normal), the D3D sampler at a given lod (tests/sampler_rule.py, T1-T3), the N64 colour combiner as the reference
generates it (rt64_shader.cpp:228-310), the material's mixes and multipliers, the tangent frame of the triangle's UVs.  It reads a `SceneData`, the texture
levels, the rays, the hits and the lods; it imports nothing from oracle/ and nothing from the library.

Every value is an `F` of tests/light_rule.py: a float64 value and a first-order bound on what a float32 evaluation of the same expression may differ by.  A texel
is the rule at the interpolated UV; its bound is the spread of the rule over the corners of the box (u +- du, v +- dv, lod +- dlod) -- du, dv the UV's own bound
plus the rounding of the sampler's texel coordinate -- widened by FILTER_EPS for the float32 arithmetic of the filter.  Discrete decisions -- the texel under a
POINT filter, the POINT level, the 0.3 thresholds, the side the ray comes from (A6), a zero vertex normal, the branch and handedness of the tangent frame -- are
taken on the value; where the margin of one is below DECISION_K x the error of its two sides the hit is *undecided* and held only to what no decision touches.
"""
import numpy as np

import light_rule as L
import sampler_rule as T
import surface_rule as S
from light_rule import F

VALID, BAD_HIT, TEXTURED, NORMAL_MAPPED, SPECULAR_MAPPED, CUTOUT, SHADOW_CUTOUT, NOISE_ALPHA, BACK_FACE = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x100
DECISION_K = L.DECISION_K
U = L.U
EDGE = float(np.float32(0.3))          # the texture-edge threshold as the float32 constant it is
# float32 arithmetic of the filter on values in 0 .. 1: byte x (1 / 255) (constant and product: 2 roundings), two lerps along x and one along y (sub, mul, add
# each, on top of each other: 9 more at most), the blend of two levels (3 more) -- 14 roundings of at most U each; taken as 24.
FILTER_EPS = 24 * U
OPT_ALPHA, OPT_EDGE, OPT_NOISE = 1 << 24, 1 << 26, 1 << 27
SHADER_NORMAL_MAP, SHADER_SPECULAR_MAP = 0x4, 0x8

MUTATIONS = ("point_level_floor", "mix_sign_swapped", "mix_on_texel_alpha", "no_detail_scale", "binormal_sign_dropped", "tangent_not_flipped",
             "shadow_by_solid_multiplier", "shadow_at_given_lod", "edge_threshold_ge", "alpha_after_noise", "separate_alpha_ignored")

FIELDS = (("color", slice(0, 4)), ("normal", slice(4, 7)), ("specular", slice(8, 11)), ("shadow", slice(11, 12)))


def shader_of(data, inst):
    """(shader id, filter, hAddr, vAddr, flags) of an instance: its own `shader` where the scene gives it one, the scene's otherwise."""
    own = getattr(inst, "shader", None)
    return tuple(own) if own is not None else (data.shader_id, data.shader_filter, data.shader_haddr, data.shader_vaddr, data.shader_flags)


def texture_levels(data, mipmaps=False):
    """texture index -> list of [h, w, 4] uint8 levels of the scene's RGBA8 textures: level 0, and with `mipmaps` the chain generate_mipmaps makes (M2-M4)."""
    import mipgen_rule
    out = {}
    for k, t in enumerate(data.textures):
        if t.format == 0x1:
            img = np.ascontiguousarray(np.asarray(t.data, dtype=np.uint8).reshape(t.height, t.width, 4))
            out[k] = mipgen_rule.chain(img) if mipmaps else [img]
    return out


def clamp_lod(lod, mips):
    """H3: clamp(lod, 0, mips - 1), NaN and negative values 0 (exact in float32: every value is the input, 0 or an integer)."""
    lod = np.asarray(lod, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(lod > 0.0, np.minimum(lod, float(mips - 1)), 0.0)


def _texel(levels, u, v, lod, filt, ha, va, point_floor=False):
    """The texture at (u, v) (F) and clamped lod [N] -> ([r, g, b, a] as F, undecided [N])."""
    mips = len(levels)
    h0, w0 = levels[0].shape[:2]
    du = u.e + 2.0 * U * np.abs(u.v); dv = v.e + 2.0 * U * np.abs(v.v)          # the UV's bound + u * w and - 0.5 of the texel coordinate, each rounded once
    dlod = U * lod                                                                  # lod + 0.5 (POINT) rounds once; lod - floor(lod) (LINEAR) is exact

    def at(uu, vv, ll):
        if point_floor and filt == T.POINT:
            lvl = np.floor(ll).astype(np.int64)
            val, tm, _ = T.sample_level(levels, uu, vv, lvl, filt, ha, va)
            return val, tm, np.full(ll.shape, np.inf), lvl
        val, tm, lm, l0, _l1, _raw = T.sample_at_lod(levels, uu, vv, ll, filt, ha, va)
        return val, tm, lm, l0
    centre, tm, lm, l0 = at(u.v, v.v, lod)
    vmin, vmax = centre.copy(), centre.copy()
    for su in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            for sl in (-1.0, 1.0):
                val = at(u.v + su * du, v.v + sv * dv, np.clip(lod + sl * dlod, 0.0, mips - 1))[0]
                vmin, vmax = np.minimum(vmin, val), np.maximum(vmax, val)
    spread = np.maximum(vmax - centre, centre - vmin) + FILTER_EPS
    undecided = np.zeros(len(lod), dtype=bool)
    if filt == T.POINT:
        w = np.maximum(w0 >> l0, 1).astype(np.float64); h = np.maximum(h0 >> l0, 1).astype(np.float64)
        undecided |= tm < DECISION_K * np.maximum(du * w, dv * h)                 # which texel
        undecided |= lm < DECISION_K * U * (lod + 0.5)                             # which level
    return [F(centre[:, c], spread[:, c]) for c in range(4)], undecided


# ---- the colour combiner, rt64_shader.cpp:228-310 ------------------------------------------------------------------------------------------

def _combiner(shader_id):
    slots = [(shader_id >> (3 * i)) & 7 for i in range(8)]
    c = [slots[0:4], slots[4:8]]
    cc = {"c": c, "alpha": bool(shader_id & OPT_ALPHA), "edge": bool(shader_id & OPT_EDGE), "noise": bool(shader_id & OPT_NOISE),
          "same": (shader_id & 0xfff) == ((shader_id >> 12) & 0xfff), "tex0": any(s in (5, 6) for s in slots),
          "inputs": max([s for s in slots if 1 <= s <= 4], default=0)}
    for i in range(2):
        cc["single%d" % i] = c[i][2] == 0
        cc["multiply%d" % i] = c[i][1] == 0 and c[i][3] == 0
        cc["mix%d" % i] = c[i][1] == c[i][3]
    return cc


def _color_input(item, with_alpha, inputs_have_alpha, hint_single, inputs, t0, t1, one, zero):
    if item == 0:
        return [zero, zero, zero, zero if with_alpha else one]
    if 1 <= item <= 4:
        x = inputs[item - 1]
        return x if (with_alpha or not inputs_have_alpha) else [x[0], x[1], x[2], one]
    if item == 5:
        return t0 if with_alpha else [t0[0], t0[1], t0[2], one]
    if item == 6:
        return [t0[3], t0[3], t0[3], t0[3] if (hint_single or with_alpha) else one]
    return t1 if with_alpha else [t1[0], t1[1], t1[2], one]


def _color_formula(cc, with_alpha, opt_alpha, inputs, t0, t1, one, zero):
    c = cc["c"][0]

    def ci(item, hint=False):
        return _color_input(item, with_alpha, opt_alpha, hint, inputs, t0, t1, one, zero)
    if cc["single0"]:
        return ci(c[3])
    if cc["multiply0"]:
        return [L.mul(a, b) for a, b in zip(ci(c[0]), ci(c[2], True))]
    if cc["mix0"]:
        return [L.lerp(x, y, s) for x, y, s in zip(ci(c[1]), ci(c[0]), ci(c[2], True))]
    s = ci(c[2], True)[0]                                                         # `.r` of the third input scales all four channels
    return [L.add(L.mul(L.sub(a, b), s), d) for a, b, d in zip(ci(c[0]), ci(c[1]), ci(c[3]))]


def _alpha_formula(cc, inputs, t0, t1, zero):
    c = cc["c"][1]

    def ai(item):
        return zero if item == 0 else inputs[item - 1][3] if item <= 4 else t0[3] if item <= 6 else t1[3]
    if cc["single1"]:
        return ai(c[3])
    if cc["multiply1"]:
        return L.mul(ai(c[0]), ai(c[2]))
    if cc["mix1"]:
        return L.lerp(ai(c[1]), ai(c[0]), ai(c[2]))
    return L.add(L.mul(L.sub(ai(c[0]), ai(c[1])), ai(c[2])), ai(c[3]))


def _combined_alpha(cc, inputs, t0, t1, one, zero, separate=True):
    if separate and not cc["same"] and cc["alpha"]:
        return _alpha_formula(cc, inputs, t0, t1, zero)
    return _color_formula(cc, cc["alpha"], cc["alpha"], inputs, t0, t1, one, zero)[3]


def _times(c, a):
    """c * a for an exact constant c: one rounding, none where a is exactly 1 (a product with 1 is exact in any binary format)."""
    r = L.mul(c, a)
    return F(r.v, np.where((a.v == 1.0) & (a.e == 0.0), 0.0, r.e))


def _threshold(a):
    """H6 / H10: value > 0.3 becomes 1.  -> (F, cutout [N], undecided [N])"""
    over = a.v > EDGE
    return L.where(over, F(np.ones_like(a.v)), a), ~over, np.abs(a.v - EDGE) < DECISION_K * a.e


def _decide_nonzero(x):
    """x != 0 as float32 evaluates it: the value's own answer, undecided where zero lies within DECISION_K x the bound (an exact zero of exact terms is decided)."""
    return x.v != 0.0, (np.abs(x.v) < DECISION_K * x.e) & (x.e > 0.0) & (x.v != 0.0)


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------

def materials(data, levels, rays, hits, lods=None, mutate=None):
    """-> dict of per-record arrays: kind (0 miss, 1 bad hit, 2 real), color (value, bound) (N, 4), normal / specular (N, 3), shadow (N, 1), flags (int64, without
    VALID / BAD_HIT logic applied to non-hits), lod (float32), undecided (bool), instance, primitive (int64)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rays = np.asarray(rays, dtype=np.float32); hits = np.asarray(hits, dtype=np.float32)
    n = len(rays)
    lods = np.zeros(n, dtype=np.float32) if lods is None else np.asarray(lods, dtype=np.float32)
    surf = S.surfaces(data, rays, hits)
    out = {"kind": surf["kind"], "instance": surf["instance"], "primitive": surf["primitive"], "undecided": surf["undecided"].copy(),
           "flags": np.zeros(n, dtype=np.int64), "lod": np.zeros(n, dtype=np.float32), "back": surf["back"]}
    for name, k in (("color", 4), ("normal", 3), ("specular", 3), ("shadow", 1)):
        out[name] = (np.zeros((n, k)), np.zeros((n, k)))
    layout = S.vertex_layout(data.shader_id)
    for k, index in enumerate(S.raytraced_instances(data)):
        I = data.instances[index]
        mesh = data.meshes[I.mesh]
        sel = np.nonzero((surf["kind"] == 2) & (surf["instance"] == k))[0]
        if not len(sel):
            continue
        m = len(sel)
        shader_id, filt, ha, va, sflags = shader_of(data, I)
        assert S.vertex_layout(shader_id) == layout, "one vertex layout per scene"
        cc = _combiner(shader_id)
        mat = I.material
        one, zero = F(np.ones(m)), F(np.zeros(m))
        und = np.zeros(m, dtype=bool)
        flags = np.full(m, VALID, dtype=np.int64) | np.where(surf["back"][sel], BACK_FACE, 0)
        u, v = F(hits[sel, 1].astype(np.float64)), F(hits[sel, 2].astype(np.float64))
        b = [L.sub(L.sub(1.0, u), v), u, v]                                       # H2
        corner = [np.asarray(mesh.indices, dtype=np.int64)[3 * surf["primitive"][sel] + c] for c in range(3)]
        # colour inputs: float3 (float4 with the alpha option) per input behind the UV; alpha 1 without the option
        stride = 16 if cc["alpha"] else 12
        first = layout["uv"] + (8 if layout["has_uv"] else 0)
        inputs = []
        for i in range(4):
            if i < cc["inputs"]:
                raw = [S._fetch(mesh, layout, corner[c], first + i * stride, 4 if cc["alpha"] else 3) for c in range(3)]
                val = S._interp(raw, b)
                inputs.append(val if cc["alpha"] else val + [one])
            else:
                inputs.append([zero, zero, zero, zero])
        uv = [F(surf["uv"][0][sel, c], surf["uv"][1][sel, c]) for c in range(2)]
        lod = lods[sel].astype(np.float64)
        mix = [float(mat.diffuseColorMix.x), float(mat.diffuseColorMix.y), float(mat.diffuseColorMix.z), float(mat.diffuseColorMix.w)]
        k_tex, k_out = max(-mix[3], 0.0), max(mix[3], 0.0)
        if mutate == "mix_sign_swapped":
            k_tex, k_out = k_out, k_tex
        t1 = [one, zero, one, one]                                                # H4's placeholder
        t0 = t0s = [zero, zero, zero, zero]
        if cc["tex0"]:
            lv = levels[I.diffuse]
            cl = clamp_lod(lod, len(lv))
            tex, ud = _texel(lv, uv[0], uv[1], cl, filt, ha, va, point_floor=(mutate == "point_level_floor"))
            und |= ud
            t0 = [L.lerp(tex[c], mix[c], k_tex) for c in range(3)] + [L.lerp(tex[3], mix[3], k_tex) if mutate == "mix_on_texel_alpha" else tex[3]]
            if mutate == "shadow_at_given_lod":
                t0s = tex
            else:
                t0s, ud = _texel(lv, uv[0], uv[1], np.zeros(m), filt, ha, va)     # H10: level 0 whatever the lod
                und |= ud
            flags |= TEXTURED
            out["lod"][sel] = cl.astype(np.float32)
        # H5
        separate = mutate != "separate_alpha_ignored"
        if separate and not cc["same"] and cc["alpha"]:
            col = _color_formula(cc, False, True, inputs, t0, t1, one, zero)
            col[3] = _alpha_formula(cc, inputs, t0, t1, zero)
        else:
            col = _color_formula(cc, cc["alpha"], cc["alpha"], inputs, t0, t1, one, zero)
        col = [L.lerp(col[c], mix[c], k_out) for c in range(3)] + [L.saturate(_times(float(mat.solidAlphaMultiplier), col[3]))]
        sa = _combined_alpha(cc, inputs, t0s, t1, one, zero)
        sa = L.saturate(_times(float(mat.solidAlphaMultiplier if mutate == "shadow_by_solid_multiplier" else mat.shadowAlphaMultiplier), sa))
        if cc["edge"]:                                                            # H6, H10
            if mutate == "edge_threshold_ge":
                over = col[3].v >= EDGE
                col[3] = L.where(over, one, col[3]); flags |= np.where(~over, CUTOUT, 0)
            else:
                col[3], cut, ud = _threshold(col[3])
                flags |= np.where(cut, CUTOUT, 0); und |= ud
            sa, cut, ud = _threshold(sa)
            flags |= np.where(cut, SHADOW_CUTOUT, 0); und |= ud
        if cc["noise"]:                                                           # H7
            flags |= NOISE_ALPHA
            if mutate == "alpha_after_noise":
                col[3] = L.mul(col[3], 0.0)
        out["color"][0][sel], out["color"][1][sel] = S._stack(col)
        out["shadow"][0][sel], out["shadow"][1][sel] = S._stack([sa])
        # H8
        normal = [F(surf["shading"][0][sel, c], surf["shading"][1][sel, c]) for c in range(3)]
        scale = 1.0 if mutate == "no_detail_scale" else float(mat.uvDetailScale)
        suv = [L.mul(uv[0], scale), L.mul(uv[1], scale)] if layout["has_uv"] else None
        if (sflags & SHADER_NORMAL_MAP) and layout["has_uv"] and I.normal is not None:
            p = [S._fetch(mesh, layout, corner[c], 0, 3) for c in range(3)]
            t = [S._fetch(mesh, layout, corner[c], layout["uv"], 2) for c in range(3)]
            nr = [S._fetch(mesh, layout, corner[c], layout["normal"], 3) for c in range(3)]
            tu = [[F(t[c][:, a]) for a in range(2)] for c in range(3)]
            uva, uvb = L.sub(tu[1][0], tu[0][0]), L.sub(tu[2][0], tu[0][0])
            uvc, uvd = L.sub(tu[1][1], tu[0][1]), L.sub(tu[2][1], tu[0][1])
            uvk = L.sub(L.mul(uvb, uvc), L.mul(uva, uvd))
            d1, d2 = L.sub3(S._vecF(p[1]), S._vecF(p[0])), L.sub3(S._vecF(p[2]), S._vecF(p[0]))
            with np.errstate(divide="ignore", invalid="ignore"):
                ta = L.normalize3(L.scale3(L.sub3(L.scale3(d2, uvc), L.scale3(d1, uvd)), L.rcp(uvk)))
                tb = L.normalize3(L.scale3(d1, L.rcp(uva)))
                tc = L.normalize3(L.scale3(d2, L.rcp(uvb)))
            (ka, ua), (kb, ub), (kc, uc) = _decide_nonzero(uvk), _decide_nonzero(uva), _decide_nonzero(uvb)
            und |= ua | (~ka & ub) | (~ka & ~kb & uc)
            tangent = [L.where(ka, ta[c], L.where(kb, tb[c], L.where(kc, tc[c], zero))) for c in range(3)]
            # handedness: z of cross((uv1 - uv0) with y negated, (uv2 - uv1) with y negated)
            e1 = [L.sub(tu[1][0], tu[0][0]), L.neg(L.sub(tu[1][1], tu[0][1]))]
            e2 = [L.sub(tu[2][0], tu[1][0]), L.neg(L.sub(tu[2][1], tu[1][1]))]
            crz = L.sub(L.mul(e1[0], e2[1]), L.mul(e1[1], e2[0]))
            und |= (np.abs(crz.v) < DECISION_K * crz.e) & (crz.e > 0.0) & (crz.v != 0.0)
            hand = np.where(crz.v < 0.0, -1.0, 1.0)
            if mutate == "binormal_sign_dropped":
                hand = np.ones(m)
            vn = S._interp(nr, b)
            is_zero = (vn[0].v == 0.0) & (vn[1].v == 0.0) & (vn[2].v == 0.0)
            tn = L.neg3(L.cross3(L.sub3(S._vecF(p[2]), S._vecF(p[0])), L.sub3(S._vecF(p[1]), S._vecF(p[0]))))
            with np.errstate(divide="ignore", invalid="ignore"):
                unit = L.normalize3(vn)
            unit = [L.where(is_zero, tn[c], unit[c]) for c in range(3)]
            binormal = [F(c.v * hand, c.e) for c in L.cross3(tangent, unit)]
            N = S._normal_matrix(np.asarray(I.transform, dtype=np.float32).astype(np.float64))
            sign = np.where(surf["back"][sel], -1.0, 1.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                tw = [F(c.v * (1.0 if mutate == "tangent_not_flipped" else sign), c.e) for c in L.normalize3(S._mul_vector(N, tangent))]
                bw = [F(c.v * sign, c.e) for c in L.normalize3(S._mul_vector(N, binormal))]
            tex, ud = _texel(levels[I.normal], suv[0], suv[1], clamp_lod(lod, len(levels[I.normal])), filt, ha, va, point_floor=(mutate == "point_level_floor"))
            und |= ud
            nc = [L.sub(L.mul(tex[c], 2.0), 1.0) for c in range(3)]
            with np.errstate(divide="ignore", invalid="ignore"):
                normal = L.normalize3(L.add3(L.add3(L.scale3(normal, nc[2]), L.scale3(tw, nc[0])), L.scale3(bw, nc[1])))
            flags |= NORMAL_MAPPED
        out["normal"][0][sel], out["normal"][1][sel] = S._stack(normal)
        # H9
        spec = [one, one, one]
        if (sflags & SHADER_SPECULAR_MAP) and layout["has_uv"] and I.specular is not None:
            tex, ud = _texel(levels[I.specular], suv[0], suv[1], clamp_lod(lod, len(levels[I.specular])), filt, ha, va, point_floor=(mutate == "point_level_floor"))
            und |= ud
            spec = tex[:3]
            flags |= SPECULAR_MAPPED
        out["specular"][0][sel], out["specular"][1][sel] = S._stack(spec)
        out["flags"][sel] = flags
        out["undecided"][sel] |= und
    return out


def as_records(rule):
    """The rule's own values in RT64_RAY_MATERIAL's layout, (N, 16) float32."""
    n = len(rule["kind"])
    rec = np.zeros((n, 16), dtype=np.float32); ri = rec.view(np.uint32)
    real = rule["kind"] == 2
    rec[:, 0:4] = rule["color"][0]; rec[:, 4:7] = rule["normal"][0]; rec[:, 8:11] = rule["specular"][0]; rec[:, 11] = rule["shadow"][0][:, 0]
    rec[:, 12] = rule["lod"]
    ri[:, 7] = np.where(real, rule["flags"], np.where(rule["kind"] == 1, BAD_HIT, 0))
    ri[:, 13] = np.where(real, rule["instance"], -1).astype(np.int64) & 0xFFFFFFFF
    ri[:, 14] = np.where(real, rule["primitive"], 0xFFFFFFFF)
    return rec


def compare(rule, got):
    """Per record: ratio |record - rule| / bound of color, normal, specular, shadow (the largest over the components; a NaN counts as inf) and whether flags, lod,
    instance, primitive and reserved are exactly the rule's.  An undecided hit is held to VALID, instance, primitive, reserved and the lod only (its ratios are 0).
    Records that are not real hits must equal the miss / bad-hit record word for word."""
    got = np.asarray(got, dtype=np.float32); gi = got.view(np.uint32)
    want = as_records(rule); wi = want.view(np.uint32)
    real = rule["kind"] == 2
    decided = real & ~rule["undecided"]
    exact = (gi[:, 13] == wi[:, 13]) & (gi[:, 14] == wi[:, 14]) & (gi[:, 15] == 0) & (gi[:, 12] == wi[:, 12])
    exact &= np.where(decided, gi[:, 7] == wi[:, 7], (gi[:, 7] & VALID) == (wi[:, 7] & VALID))
    exact &= real | (gi == wi).all(axis=1)
    ratios = {}
    for name, cols in FIELDS:
        v, e = rule[name]
        diff = np.abs(got[:, cols].astype(np.float64) - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff == 0.0, 0.0, diff / e)
        r = np.where(np.isnan(r), np.inf, r).max(axis=1)
        ratios[name] = np.where(decided, r, 0.0)
    return ratios, exact


def report(name, rule, ratios, exact):
    """One line per case, laid out like profiles/surface_rule_deviation.txt."""
    real = rule["kind"] == 2
    n = int(real.sum())
    parts = ["%-34s hits %5d of %5d" % (name, n, len(real))]
    for k, _ in FIELDS:
        r = ratios[k][real]
        parts.append("%s max %.3f mean %.4f" % (k, r.max() if n else 0.0, r.mean() if n else 0.0))
    parts.append("undecided %.4f" % (float(rule["undecided"][real].mean()) if n else 0.0))
    parts.append("inexact %d" % int((~exact).sum()))
    return "  ".join(parts)
