"""One reflection pass and the refraction pass as rules in numpy float64 (rules M1-M12 and G1-G6).  TEST INFRASTRUCTURE.

`reflection_kernel` and `refraction_kernel` (csrc/passes.hip) and their C restatements in oracle/oracle_render.c were written from the same HLSL by the same hand.
This module states the two operations a third time, from their meaning (ReflectionRayGen.hlsl:25-143, RefractionRayGen.hlsl:19-117), in float64, with
the `F` arithmetic of tests/light_rule.py: every value carries a first-order bound on what a float32 evaluation may differ by, every discrete decision is taken on the
value, and a pixel whose decision has a margin below DECISION_K x the error of its two sides is reported undecided instead of guessed.  It imports nothing from oracle/.

A pass reads what is STORED: position (float32), view direction and normal (f16 values), instance id, the REFLECTION / REFRACTION image (alpha = the pass's weight).
It predicts the image after the pass and, for a mirror, the continuation state the next pass starts from.  Errors never compound across passes: the rule for pass
k + 1 starts again from what pass k stored.

Reference lines cited as (M:n) are ReflectionRayGen.hlsl, (G:n) RefractionRayGen.hlsl, (Fog:n) Fog.hlsli, (I:n) Instances.hlsli.

The sky a ray leaves into is tests/sky_rule.py's (E1-E8) where `scene["sky"]` is a sky description -- along the mirror ray, at the pixel's screen UV behind glass --
else the one constant term of a scene whose sky texels are all equal.

Out of scope: normal and specular maps, texture gradients other than zero (a secondary ray carries none: level 0), the hit list past 16 entries, background instances.
"""
import numpy as np

import light_rule as L
import sky_rule as S
from light_rule import F

EPSILON = L.EPSILON
DECISION_K = L.DECISION_K
RAY_MAX_DISTANCE = 100000.0                         # Ray.hlsli:10
SNORM16_HALF_STEP = 0.5 / 32767.0
TIE = 2.0 ** -10                                    # a UNORM8 rounding is a decision: x * 255 must stay this far from k + 0.5 (float32 puts it within 2^-15)
HIGHLIGHT = [float(np.float32(x)) for x in (1.0, 1.05, 1.2)]          # (M:131-132)
SHADOW = [float(np.float32(x)) for x in (0.1, 0.05, 0.0)]
MAX_HITS = 16
# "alpha above EPSILON" is asked of the f16 that is stored: 1e-6 lies between 16 and 17 subnormal steps of 2^-24, so the stored value is above it from 16.5 steps on
GOES_ON = 16.5 * 2.0 ** -24

MUTATIONS = ("fresnel_from_hit", "fresnel_no_floor", "mirror_fog_from_camera", "mirror_shadows", "glass_no_shadows", "eye_light", "direction_normalised",
             "k_unsaturated", "shine_abs", "state_without_hit", "state_first_hit", "state_lit_only", "eta_inverted", "tir_ignored", "order_by_t", "light_slot_plus_one", "no_flip", "texel_point")


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------

def take(f, idx):
    return F(f.v[idx], f.e[idx])


def put(dst, mask, src):
    """dst where ~mask, src (already of mask.sum() values) where mask."""
    v = dst.v.copy(); e = np.array(dst.e, dtype=np.float64); v[mask] = src.v; e[mask] = src.e
    return F(v, e)


def unorm8(x):
    """A material constant in [0, 1] as the hit record's RGBA8 stores it: (value k / 255 as F, tie): k = round(255 x); tie where float32 could round the other way."""
    y = np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0) * 255.0
    k = np.rint(y)
    tie = np.abs(np.abs(y - np.floor(y)) - 0.5) < TIE
    v = k / 255.0
    return F(v, np.where((k == 0) | (k == 255), 0.0, 2.0 * L.U * v)), tie


def fmin(a, c):
    v = np.minimum(a.v, c)
    return F(v, np.maximum(np.minimum(a.v + a.e, c) - v, v - np.minimum(a.v - a.e, c)))


def clamp(a, lo, hi):
    return fmin(L.fmax(a, lo), hi)


def scene_triangles(scene):
    """All triangles of the ray-traced instances, concatenated: (v0, e1, e2 (T, 3), instance (T,), index within the instance (T,))."""
    v0, e1, e2, inst, prim = [], [], [], [], []
    for k, I in enumerate(scene["instances"]):
        t = np.asarray(I["triangles"], dtype=np.float64).reshape(-1, 3, 3)
        v0.append(t[:, 0]); e1.append(t[:, 1] - t[:, 0]); e2.append(t[:, 2] - t[:, 0]); inst.append(np.full(len(t), k)); prim.append(np.arange(len(t)))
    return np.concatenate(v0), np.concatenate(e1), np.concatenate(e2), np.concatenate(inst), np.concatenate(prim)


# ---- the hit list (M2-M3) --------------------------------------------------------------------------------------------------------------------

def hit_lists(scene, origin, direction, mutate=None, chunk=512, origin_e=None, direction_e=None):
    """Every ray against every triangle, float64 brute force (light_rule.triangle_test, margins of BruteForceShadows).  A hit needs tmin 0.1 < t < 100000 and, unless
    its instance disables culling, a front face: det = e1 . (d x e2) > 0.  Hits are ordered by t - depthBias (I:17-19).
    origin_e (N,), direction_e (N, 3): by how much a ray's origin (a length) and direction (per component) may themselves be off (a ray that starts from computed
    values, tests/gi_rule.py); they widen the margins to first order: the numerators of u, v, t move by at most |do| |d| |e| + |tv| |dd| |e|, det by |dd| |e1| |e2|.
    With them a ray parallel to a triangle's plane, exactly or beyond the triangle's reach, is a decided miss (the two tests are explained where they stand).

    Returns dict: count (N,), decided (N,) -- every triangle a decided hit or a decided miss -- and per slot (N, M): tri (index into scene_triangles), u, v, t, du, dv, dt,
    key, key_e, front (bool), front_decided (bool)."""
    v0, e1, e2, inst, _ = scene_triangles(scene)
    cull = np.asarray([bool(I["cull"]) for I in scene["instances"]])[inst]
    bias = np.asarray([float(I["material"]["depthBias"]) for I in scene["instances"]])[inst]
    n = len(origin)
    l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    out = {k: [] for k in ("tri", "u", "v", "t", "du", "dv", "dt", "key", "key_e", "front", "front_decided")}
    counts, decided = np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool)
    for a in range(0, n, chunk):
        o, d = origin[a:a + chunk], direction[a:a + chunk]
        u, v, t, du, dv, dt, det, ok = L.triangle_test(v0, e1, e2, o, d)
        w = 1.0 - u - v
        det_e = L.SHADOW_K * L.U * np.linalg.norm(d, axis=1)[:, None] * (l1 * l2)[None]
        parallel = np.zeros(det.shape, dtype=bool)
        if origin_e is not None:
            oe, dc = np.asarray(origin_e)[a:a + chunk, None], np.abs(np.asarray(direction_e)[a:a + chunk])
            de = np.linalg.norm(dc, axis=1)[:, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / np.abs(det)
                move = oe * np.linalg.norm(d, axis=1)[:, None] + np.linalg.norm(o[:, None, :] - v0[None], axis=2) * de
                rel = de * (l1 * l2)[None] * inv
                du = du + move * l2[None] * inv + np.abs(u) * rel
                dv = dv + move * l1[None] * inv + np.abs(v) * rel
                dt = dt + oe * (l1 * l2)[None] * inv + np.abs(t) * rel
            ok = ok & np.isfinite(du) & np.isfinite(dv) & np.isfinite(dt)
            det_e = det_e + de * (l1 * l2)[None]
            # det = e1 . (d x e2) is a sum of six products e1_i d_j e2_k.  Where every one of them has a factor that is exactly zero (a ray along an axis-aligned face: the
            # component of d itself and its error are zero) every float32 evaluation gives 0 too, and det == 0 is a miss (oracle_trace.c R3; an exact parallel never meets the plane)
            a1, a2, ad = np.abs(e1)[None], np.abs(e2)[None], (np.abs(d) + dc)[:, None, :]
            size = sum(a1[..., i] * (ad[..., j] * a2[..., k] + ad[..., k] * a2[..., j]) for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)))
            parallel = size == 0.0
            # a ray all but parallel to a triangle's plane whose sign of det float32 cannot tell: it meets the plane no nearer than |t| >= (|num| - its error) / (|det| +
            # its error), num = e2 . (tv x e1); a triangle reaches no farther from the origin than |tv| + |e1| + |e2|: beyond that, a miss whatever the sign
            tvv = o[:, None, :] - v0[None]
            T = np.linalg.norm(tvv, axis=2)
            num = np.abs(np.einsum("ntk,ntk->nt", np.broadcast_to(e2[None], tvv.shape), np.cross(tvv, e1[None])))
            num_e = (L.SHADOW_K * L.U * (T + (np.linalg.norm(o, axis=1)[:, None] + np.linalg.norm(v0, axis=1)[None]) / L.SHADOW_K) + oe) * (l1 * l2)[None]
            parallel |= (num - num_e) * np.linalg.norm(d, axis=1)[:, None] > (np.abs(det) + det_e) * 2.0 * (T + (l1 + l2)[None])
        front, front_dec = det > 0.0, np.abs(det) > det_e
        facing_ok = ~cull[None] | (front & front_dec)
        facing_no = cull[None] & ~front & front_dec
        inside = (u > du) & (v > dv) & (w > du + dv) & (t > L.RAY_MIN_DISTANCE + dt) & (t < RAY_MAX_DISTANCE - dt)
        outside = (u < -du) | (v < -dv) | (w < -(du + dv)) | (t < L.RAY_MIN_DISTANCE - dt) | (t > RAY_MAX_DISTANCE + dt)
        hit = ok & inside & facing_ok & ~parallel
        miss = (ok & outside) | facing_no | parallel          # (a ray within rounding of a triangle's plane is decided only by another test)
        decided[a:a + chunk] = (hit | miss).all(axis=1)
        counts[a:a + chunk] = hit.sum(axis=1)
        key = np.where(hit, (t if mutate == "order_by_t" else t - bias[None]), np.inf)
        m = max(int(hit.sum(axis=1).max()) if len(o) else 0, 1)
        order = np.argsort(key, axis=1, kind="stable")[:, :m]
        rows = np.arange(len(o))[:, None]
        got = {"tri": order, "u": u[rows, order], "v": v[rows, order], "t": t[rows, order], "du": du[rows, order], "dv": dv[rows, order], "dt": dt[rows, order],
               "key": key[rows, order], "front": front[rows, order], "front_decided": front_dec[rows, order]}
        got["key_e"] = got["dt"] + L.U * (np.abs(got["t"]) + np.abs(bias[order]))
        for k in out:
            out[k].append(got[k])
    width = max([x.shape[1] for x in out["tri"]] + [1])

    def pad(xs, fill):
        return np.concatenate([np.pad(x, ((0, 0), (0, width - x.shape[1])), constant_values=fill) for x in xs], axis=0) if xs else np.zeros((0, width))
    res = {k: pad(v, np.inf if k == "key" else 0) for k, v in out.items()}
    res["count"], res["decided"] = counts, decided
    return res


def hit_normals(scene, tri, u, v, du, dv, front):
    """Shading normal of hits (one per ray): the vertex normals interpolated by (1 - u - v, u, v), through the instance's normal matrix, renormalised, turned against the
    ray (rt64_shader.cpp:518-521; tests/surface_rule.py A7), then SNORM16: the value is kept unrounded and the bound takes half a step."""
    import surface_rule as S
    _, _, _, inst, prim = scene_triangles(scene)
    n = len(tri)
    out = [F(np.zeros(n)) for _ in range(3)]
    for k, I in enumerate(scene["instances"]):
        sel = np.nonzero(inst[tri] == k)[0]
        if not len(sel):
            continue
        nr = np.asarray(I["normals"], dtype=np.float64).reshape(-1, 3, 3)[prim[tri[sel]]]
        # (1 - u - v) n0 + u n1 + v n2 = n0 + u (n1 - n0) + v (n2 - n0): the errors of u and v reach the normal through the differences of the corners' normals only (none on
        # a flat face); the float32 evaluation of the three products and two sums on exact u, v is the F arithmetic's
        b = [L.sub(L.sub(1.0, F(u[sel])), F(v[sel])), F(u[sel]), F(v[sel])]
        vn = S._interp([nr[:, 0], nr[:, 1], nr[:, 2]], b)
        vn = [F(vn[c].v, vn[c].e + np.abs(nr[:, 1, c] - nr[:, 0, c]) * du[sel] + np.abs(nr[:, 2, c] - nr[:, 0, c]) * dv[sel]) for c in range(3)]
        N = S._normal_matrix(np.asarray(I["transform"], dtype=np.float32).astype(np.float64))
        sn = L.normalize3(S._mul_vector(N, L.normalize3(vn)))
        sign = np.where(front[sel], 1.0, -1.0)
        for c in range(3):
            x = F(sn[c].v * sign, sn[c].e + SNORM16_HALF_STEP)
            out[c] = put(out[c], inst[tri] == k, x)
    return out


def hit_colours(scene, tri, u, v, du, dv, mutate=None):
    """Colour of hits as the hit record's RGBA8 holds it: three F, a tie mask and which hits took a texel.  diffuseColorMix.w = 1: the mix colour.  w = 0 on an instance
    with a `texture` (levels, uv (T, 3, 2), filter, ha, va): the texel of tests/sampler_rule.py at zero gradients (lod 0) at the interpolated uv, whose error is that of the
    barycentrics through the corners' uv differences; `sample_grad_bounds` gives the lowest and highest byte a float32 sampler may store over that box, and the colour is
    their middle with half their distance as its error (one byte: the UNORM8 value itself)."""
    import sampler_rule as SR
    _, _, _, inst, prim = scene_triangles(scene)
    n = len(tri)
    col = [F(np.zeros(n)) for _ in range(3)]
    tie = np.zeros(n, dtype=bool); textured = np.zeros(n, dtype=bool)
    for k, I in enumerate(scene["instances"]):
        here = inst[tri] == k
        if not here.any():
            continue
        mix = I["material"]["diffuseColorMix"]
        if mix[3] == 1.0:
            for c in range(3):
                q, t = unorm8(np.full(int(here.sum()), mix[c])); col[c] = put(col[c], here, q); tie[here] |= t
            continue
        T = I.get("texture")
        assert mix[3] == 0.0 and T is not None, "a surface takes its colour from diffuseColorMix with w = 1, or from its texture with w = 0"
        uv = np.asarray(T["uv"], dtype=np.float64)[prim[tri[here]]]                      # (n, 3, 2)
        uu, vv = u[here], v[here]
        tu = (1.0 - uu - vv)[:, None] * uv[:, 0] + uu[:, None] * uv[:, 1] + vv[:, None] * uv[:, 2]
        te = np.abs(uv[:, 1] - uv[:, 0]) * du[here][:, None] + np.abs(uv[:, 2] - uv[:, 0]) * dv[here][:, None] + 8.0 * L.U * np.abs(uv).max(axis=1)
        zero = np.zeros((len(tu), 2))
        r = SR.sample_grad_bounds(T["levels"], tu[:, 0], tu[:, 1], zero, zero, SR.POINT if mutate == "texel_point" else T["filter"], T["ha"], T["va"], te[:, 0], te[:, 1], 0.0, 8.0 * L.U)
        lo, hi = r["lo"].astype(np.float64), r["hi"].astype(np.float64)
        for c in range(3):
            mid = 0.5 * (lo[:, c] + hi[:, c]) / 255.0
            col[c] = put(col[c], here, F(mid, 0.5 * (hi[:, c] - lo[:, c]) / 255.0 + 2.0 * L.U * mid))
        textured[here] = True
    return col, tie, textured


# ---- fog (Fog:5-27) --------------------------------------------------------------------------------------------------------------------------

def fog_from_origin(position, origin, mul_, offset):
    distance = L.length3(L.sub3(position, origin))
    return L.saturate(L.mul(L.div(L.add(distance, offset), mul_), 0.5))


def fog_from_camera(position, view_proj, mul_, offset):
    """(Fog:5-18) clip = p * viewProj; z = 2 z - w; alpha = saturate((z / max(w, 0.001) * fogMul + fogOffset) / 255).  viewProj: 4 x 4 float64; its float32 entries are taken as
    CAM_K roundings off.  The position's own error moves clip.z and clip.w together, so it is taken through the quotient's gradient (first order, as every bound here)
    instead of through the two sums separately; the roundings of the evaluation are those of the F arithmetic on the position's value."""
    M = [[F(np.float64(view_proj[r][c]), L.CAM_K * L.U * abs(view_proj[r][c])) for c in range(4)] for r in range(4)]
    p = [F(c.v) for c in position]
    clip = [L.add(L.add(L.add(L.mul(p[0], M[0][c]), L.mul(p[1], M[1][c])), L.mul(p[2], M[2][c])), M[3][c]) for c in range(4)]
    z = L.sub(L.mul(clip[2], 2.0), clip[3])
    w = L.fmax(clip[3], float(np.float32(0.001)))
    q = L.mul(z, L.rcp(w))
    grad = sum(np.abs((2.0 * view_proj[c][2] - view_proj[c][3]) / w.v - z.v * view_proj[c][3] / (w.v * w.v)) * position[c].e for c in range(3))
    q = F(q.v, q.e + grad)
    return L.saturate(L.div(L.add(L.mul(q, mul_), offset), 255.0))


# ---- the resolve loop shared by the two passes -------------------------------------------------------------------------------------------------

def _resolve(scene, origin, direction, alpha_in, parent_inst, glass, mutate):
    """The hit list of every ray and the loop over it (M4-M8, G3-G4).  origin: three F; direction: three F; alpha_in: F (the pass's weight); parent_inst: instance id of the
    surface each ray leaves.  Returns a dict of per-ray results."""
    n = len(alpha_in.v)
    o_v = np.stack([c.v for c in origin], axis=-1); d_v = np.stack([c.v for c in direction], axis=-1)
    live = np.linalg.norm(d_v, axis=1) > 0.0                       # a zero direction (total internal reflection) meets nothing
    why = {k: np.zeros(n, dtype=bool) for k in ("hit", "order", "facing", "gate", "tie")}
    hl = hit_lists(scene, o_v[live], d_v[live], mutate=mutate) if live.any() else None
    count = np.zeros(n, dtype=np.int64)
    if hl is not None:
        count[live] = hl["count"]; why["hit"][live] = ~hl["decided"]
    M = int(count.max()) if n else 0
    assert M <= MAX_HITS, "the hit list past 16 entries is out of scope"
    inst_of_tri = scene_triangles(scene)[3]
    mats = scene["instances"]
    tab = lambda key: np.asarray([m["material"][key] for m in mats], dtype=np.float64)
    res_rgb = [F(np.zeros(n)) for _ in range(3)]; res_a = F(np.ones(n))
    transparent = [F(np.zeros(n)) for _ in range(3)]
    new_alpha = F(np.zeros(n))
    st_pos = [F(np.zeros(n)) for _ in range(3)]; st_nrm = [F(np.zeros(n)) for _ in range(3)]; st_spec = [F(np.zeros(n)) for _ in range(3)]
    st_id = np.full(n, -1, dtype=np.int64)
    contributing = np.zeros(n, dtype=np.int64); textured = np.zeros(n, dtype=bool)
    alive = count > 0
    ambient = [L.add(float(scene["ambientBase"][c]), float(scene["ambientNoGI"][c])) for c in range(3)]
    live_idx = np.nonzero(live)[0]
    parent_fresnel = tab("reflectionFresnelFactor")[parent_inst]
    for m in range(M):
        has = alive & (count > m)
        if not has.any():
            break
        rows = np.nonzero(has)[0]
        lr = np.searchsorted(live_idx, rows)                     # rows of the hit list
        g = lambda k: hl[k][lr, m]
        if M > m + 1:                                            # the order of two decided hits: separated by more than their errors (a tie keeps the first come, which no rule knows)
            nxt = count[rows] > m + 1
            gap = np.where(nxt, hl["key"][lr, m + 1] - hl["key"][lr, m], np.inf)
            why["order"][rows] |= gap <= hl["key_e"][lr, m] + np.where(nxt, hl["key_e"][lr, m + 1], 0.0)
        tri = g("tri").astype(np.int64); inst = inst_of_tri[tri]
        culled = np.asarray([bool(I["cull"]) for I in mats])[inst]
        why["facing"][rows] |= ~culled & ~g("front_decided").astype(bool)
        k = len(rows)
        # colour and alpha as the hit record holds them (UNORM8)
        col, tie, tex_here = hit_colours(scene, tri, g("u"), g("v"), g("du"), g("dv"), mutate)
        why["tie"][rows] |= tie
        tex_seen = tex_here
        h_alpha, tie = unorm8(tab("solidAlphaMultiplier")[inst]); why["tie"][rows] |= tie
        ra = take(res_a, rows)
        contrib = L.mul(ra, h_alpha)
        why["gate"][rows] |= np.abs(contrib.v - EPSILON) < DECISION_K * contrib.e
        passes = contrib.v >= EPSILON                                                                              # (M:75-76)
        # where the hit lies: origin + direction * ((t - bias) + bias)
        tF = F(g("t"), g("dt") + 2.0 * L.U * np.abs(g("t")))
        d_r = [take(c, rows) for c in direction]; o_r = [take(c, rows) for c in origin]
        pos = L.add3(o_r, L.scale3(d_r, tF))
        nrm = hit_normals(scene, tri, g("u"), g("v"), g("du"), g("dv"), g("front").astype(bool) | culled | (mutate == "no_flip"))
        spec = [L.mul(F(np.asarray([m_["material"]["specularColor"][c] for m_ in mats], dtype=np.float64)[inst]), 1.0) for c in range(3)]
        fog_on = tab("fogEnabled")[inst] != 0
        if fog_on.any():                                                                                          # (M:82-86, G:78-82)
            fm, fo = np.where(fog_on, tab("fogMul")[inst], 1.0), np.where(fog_on, tab("fogOffset")[inst], 0.0)
            from_camera = glass != (mutate == "mirror_fog_from_camera")
            fa = fog_from_camera(pos, scene["viewProj"], fm, fo) if from_camera else fog_from_origin(pos, o_r, fm, fo)
            fa = L.where(fog_on, fa, 0.0)
            fc = np.asarray([m_["material"]["fogColor"] for m_ in mats], dtype=np.float64)[inst]
            add_t = [L.mul(F(fc[:, c]), L.mul(fa, contrib)) for c in range(3)]
            contrib_f = L.where(fog_on, L.mul(contrib, L.sub(1.0, fa)), contrib)
        else:
            add_t = [F(np.zeros(k)) for _ in range(3)]; contrib_f = contrib
        lit = np.asarray([int(m_["material"]["lightGroupMaskBits"]) for m_ in mats], dtype=np.int64)[inst] > 0        # (M:78)
        self_light = np.asarray([m_["material"]["selfLight"] for m_ in mats], dtype=np.float64)[inst]
        na = take(new_alpha, rows)
        if not glass:                                                                                             # (M:19-23, 91-96)
            rf = tab("reflectionFactor")[inst]
            mirrors = rf > EPSILON
            ff = tab("reflectionFresnelFactor")[inst] if mutate == "fresnel_from_hit" else parent_fresnel[rows]    # sic: the MIRRORING instance's factor (M:93)
            base = L.add(1.0, L.dot3(nrm, d_r))
            ret = L.power(clamp(base, EPSILON, 1.0), 5.0)
            if mutate == "fresnel_no_floor":                                                                       # pow of a negative base is not a number in HLSL
                ret = F(np.where(base.v < 0.0, np.nan, ret.v), ret.e)
            fres = L.add(rf, L.mul(L.mul(L.sub(1.0, rf), ret), ff))
            na = L.where(passes & mirrors, L.add(na, L.mul(L.mul(fres, contrib_f), take(alpha_in, rows))), na)
        new_rgb, new_t = [], []
        for c in range(3):
            r_c, t_c = take(res_rgb[c], rows), take(transparent[c], rows)
            t_c = L.where(passes, L.add(t_c, add_t[c]), t_c)
            lit_add = L.add(r_c, L.mul(col[c], contrib_f))
            unlit_add = L.add(t_c, L.mul(L.mul(col[c], contrib_f), L.add(ambient[c], F(self_light[:, c]))))
            new_rgb.append(L.where(passes & lit, lit_add, r_c)); new_t.append(L.where(passes & ~lit, unlit_add, t_c))
        keeps = passes & lit if (glass or mutate == "state_lit_only") else passes                                  # (M:105-108: every contributing hit; G:84-93: the lit ones)
        if mutate == "state_first_hit":
            keeps = keeps & (st_id[rows] < 0)
        ra_new = L.where(passes, L.mul(ra, L.sub(1.0, h_alpha)), ra)
        # write back
        for c in range(3):
            res_rgb[c] = put(res_rgb[c], has, new_rgb[c]); transparent[c] = put(transparent[c], has, new_t[c])
            st_pos[c] = put(st_pos[c], has, L.where(keeps, pos[c], take(st_pos[c], rows)))
            st_nrm[c] = put(st_nrm[c], has, L.where(keeps, nrm[c], take(st_nrm[c], rows)))
            st_spec[c] = put(st_spec[c], has, L.where(keeps, spec[c], take(st_spec[c], rows)))
        st_id[rows] = np.where(keeps, inst, st_id[rows])
        contributing[rows] += passes; textured[rows] |= passes & tex_seen
        new_alpha = put(new_alpha, has, na)
        res_a = put(res_a, has, ra_new)
        why["gate"][rows] |= passes & (np.abs(ra_new.v - EPSILON) < DECISION_K * ra_new.e)
        stop = np.zeros(n, dtype=bool); stop[rows] = ra_new.v <= EPSILON                                           # (M:112)
        alive = alive & ~stop
    return dict(rgb=res_rgb, a=res_a, transparent=transparent, new_alpha=new_alpha, pos=st_pos, nrm=st_nrm, spec=st_spec, id=st_id, contributing=contributing, textured=textured,
                count=count, why=why, ambient=ambient)


def _lights(scene, R, direction, px, py, check_shadows, mutate):
    """directLight of the surface the loop ended on: one random light + selfLight (M:117-119, G:106-108).  Returns (three F for every ray, undecided by kind, rays with a surface)."""
    n = len(R["id"])
    have = R["id"] >= 0
    idx = np.nonzero(have)[0]
    light = [F(np.zeros(n)) for _ in range(3)]
    why = {k: np.zeros(n, dtype=bool) for k in ("admission", "walk", "shadow", "bound")}
    if not len(idx):
        return light, why, have
    ids = R["id"][idx]
    mats = [I["material"] for I in scene["instances"]]
    tab = lambda key: np.asarray([m[key] for m in mats], dtype=np.float64)[ids]
    st = {"position": [take(c, idx) for c in R["pos"]], "normal": [take(c, idx) for c in R["nrm"]], "specular": [take(c, idx) for c in R["spec"]],
          "rayDirection": [take(c, idx) for c in direction], "px": px[idx], "py": py[idx], "bluenoise": scene["bluenoise"], "frameCount": int(scene["frameCount"]),
          "diSamples": int(scene["diSamples"]), "shadow": scene.get("shadow"), "checkShadows": check_shadows,
          "ignoreNormalFactor": tab("ignoreNormalFactor"), "specularExponent": tab("specularExponent"), "shadowRayBias": tab("shadowRayBias")}
    mask = np.asarray([int(m["lightGroupMaskBits"]) for m in mats], dtype=np.uint32)[ids]
    res, w, _, _, _, _ = L.light_loop(st, mask, scene["lights"], 1, mutate="select_slot_plus_one" if mutate == "light_slot_plus_one" else None)
    self_light = np.asarray([m["selfLight"] for m in mats], dtype=np.float64)[ids]
    res = [L.add(a, F(self_light[:, c])) for c, a in enumerate(res)]
    if mutate == "eye_light":
        nrm, rd = st["normal"], st["rayDirection"]
        lam = L.fmax(L.dot3(nrm, L.neg3(rd)), 0.0)
        res = [L.add(a, L.mul(float(scene["eyeDiffuse"][c]), lam)) for c, a in enumerate(res)]
    for c in range(3):
        light[c] = put(light[c], have, res[c])
    for k in why:
        why[k][idx] = w[k]
    return light, why, have


def _images(h, w, active, values, errors):
    value = np.zeros((h, w, 4)); bound = np.zeros((h, w, 4))
    v = np.stack(values, axis=-1); e = np.stack(errors, axis=-1)
    value[active] = v
    bound[active] = e + np.maximum(L.F16_HALF_STEP * (np.abs(v) + e), L.F16_FLOOR)      # RGBA16F: half a step of what the device holds, never less than half a subnormal step
    return value, bound


def _f16_state(fs):
    v = np.stack([c.v for c in fs], axis=-1); e = np.stack([np.broadcast_to(c.e, c.v.shape) for c in fs], axis=-1)
    return v, e + np.maximum(L.F16_HALF_STEP * (np.abs(v) + e), L.F16_FLOOR)


# ---- one reflection pass (M1-M12) --------------------------------------------------------------------------------------------------------------

def reflection_pass(scene, position, view, normal, instance_id, reflection, mutate=None):
    """ReflectionRayGen for every pixel of a frame.  position, view, normal: (H, W, >= 3) as stored; instance_id: (H, W) int; reflection: (H, W, 4) as stored before the pass.

    scene: instances (in instance-id order: material dict, world-space triangles (T, 3, 3), object-space vertex normals (T, 3, 3), transform, cull), lights, ambientBase,
    ambientNoGI, sky (the one sky term, or zeros), bluenoise, frameCount, diSamples, viewProj (only a fog taken from the camera reads it), eyeDiffuse.
    Returns a dict: value, bound (H, W, 4) of the REFLECTION image after the pass (|stored - value| <= bound is claimed at every decided pixel; pixels the pass skips keep
    their stored value, bound 0), decided, takes (the pixels the pass works on), has_hit, state_position / _direction / _normal (value, bound) and state_id where has_hit,
    goes_on (alpha after the pass above EPSILON as an f16), info."""
    assert mutate is None or mutate in MUTATIONS, mutate
    instance_id = np.asarray(instance_id); h, w = instance_id.shape
    refl = np.asarray(reflection, dtype=np.float64)
    takes = (instance_id >= 0) & (refl[..., 3] > EPSILON)                                                  # (M:29-33)
    py, px = np.nonzero(takes)
    n = len(px)
    origin = L.vec(np.asarray(position, dtype=np.float64)[takes][:, :3])
    v = L.vec(np.asarray(view, dtype=np.float64)[takes][:, :3]); nr = L.vec(np.asarray(normal, dtype=np.float64)[takes][:, :3])
    d = L.reflect3(v, nr)                                                                                   # (M:39) not normalised
    if mutate == "direction_normalised":
        d = L.normalize3(d)
    alpha = F(refl[takes][:, 3])
    ids = instance_id[takes].astype(np.int64)
    R = _resolve(scene, origin, d, alpha, ids, False, mutate)
    light, lwhy, have = _lights(scene, R, d, px, py, mutate == "mirror_shadows", mutate)
    sky = scene["sky"]
    if S.described(sky):                                                                                    # SampleSkyPlane along the mirror ray, over no background (E1-E6)
        sky = S.over_background([F(np.zeros(n)) for _ in range(3)], S.plane_colour(sky, d), sky.get("mutate"))
    shine = np.asarray([I["material"]["reflectionShineFactor"] for I in scene["instances"]], dtype=np.float64)[ids]
    up = L.fmax(d[1], 0.0) if mutate != "shine_abs" else F(np.abs(d[1].v), d[1].e)
    down = L.fmax(L.neg(d[1]), 0.0) if mutate != "shine_abs" else F(np.abs(d[1].v), d[1].e)
    s_up, s_down = L.power(L.mul(up, shine), 3.0), L.power(L.mul(down, shine), 3.0)                          # (M:135-136)
    na = R["new_alpha"]
    k = L.mul(alpha, L.saturate(L.sub(1.0, na)) if mutate != "k_unsaturated" else L.sub(1.0, na))          # (M:139)
    vals, errs = [], []
    for c in range(3):
        rgb = L.where(have, L.mul(R["rgb"][c], L.add(R["ambient"][c], light[c])), R["rgb"][c])              # (M:119)
        rgb = L.add(rgb, L.add(L.mul(sky[c], R["a"]), R["transparent"][c]))                                # (M:127)
        rgb = L.lerp(rgb, HIGHLIGHT[c], s_up); rgb = L.lerp(rgb, SHADOW[c], s_down)
        out = L.add(F(refl[takes][:, c]), L.mul(rgb, k))                                                    # (M:139, 142)
        vals.append(out.v); errs.append(np.array(out.e))
    a_out = L.saturate(na)
    vals.append(a_out.v); errs.append(np.array(a_out.e))
    value, bound = _images(h, w, takes, vals, errs)
    value[~takes] = refl[~takes]
    # the continuation state (M:120-123) and who goes on
    has_hit = have if mutate != "state_without_hit" else np.ones(n, dtype=bool)
    goes = a_out.v >= GOES_ON
    why = dict(R["why"]); why.update({"light_" + k_: v_ for k_, v_ in lwhy.items()})
    why["goes_on"] = np.abs(a_out.v - GOES_ON) < DECISION_K * a_out.e
    why["bound"] = np.isinf(bound[takes]).any(axis=-1)             # no finite bound (an error interval that reaches a pole): not claimed; a NaN is claimed, and wrong
    und = np.zeros(n, dtype=bool)
    for x in why.values():
        und |= x
    decided = np.ones((h, w), dtype=bool); decided[takes] = ~und

    def full(x, fill=0):
        a = np.full((h, w) + x.shape[1:], fill, dtype=x.dtype); a[takes] = x; return a
    pos_v = np.stack([c.v for c in R["pos"]], axis=-1); pos_e = np.stack([np.broadcast_to(c.e, c.v.shape) for c in R["pos"]], axis=-1)
    dir_v, dir_b = _f16_state(d); nrm_v, nrm_b = _f16_state(R["nrm"])
    return dict(value=value, bound=bound, decided=decided, takes=takes, has_hit=full(has_hit), goes_on=full(goes),
                state_position=(full(pos_v), full(pos_e + L.U * np.abs(pos_v))), state_direction=(full(dir_v), full(dir_b)), state_normal=(full(nrm_v), full(nrm_b)),
                state_id=full(R["id"], -1),
                info=dict(hits=full(R["count"]), contributing=full(R["contributing"]), textured=full(R["textured"]), lit_surface=full(have), sky=full(R["a"].v > 0.0),
                          undecided={k_: int(v_.sum()) for k_, v_ in why.items()}, fresnel_alpha=full(na.v)))


# ---- the refraction pass (G1-G6) ---------------------------------------------------------------------------------------------------------------

def hlsl_refract(i, n, eta, mutate=None):
    """refract(i, n, eta) of HLSL: k = 1 - eta^2 (1 - (n . i)^2); k < 0 -> 0, else eta i - (eta (n . i) + sqrt k) n.  Returns (three F, total internal (bool), undecided)."""
    if mutate == "eta_inverted":
        eta = 1.0 / np.asarray(eta, dtype=np.float64)
    cosi = L.dot3(n, i)
    k = L.sub(1.0, L.mul(L.mul(eta, eta), L.sub(1.0, L.mul(cosi, cosi))))
    total = k.v < 0.0
    undecided = np.abs(k.v) < DECISION_K * k.e
    if mutate == "tir_ignored":                                          # the branch left out, the root taken of |k|: a ray that goes on into the surface
        total = np.zeros_like(total); k = F(np.abs(k.v), k.e)
    s = L.add(L.mul(eta, cosi), L.sqrt(L.fmax(k, 0.0)))
    out = [L.where(total, 0.0, L.sub(L.mul(i[c], eta), L.mul(n[c], s))) for c in range(3)]
    return out, total, undecided


def refraction_pass(scene, position, view, normal, instance_id, refraction, mutate=None):
    """RefractionRayGen for every pixel of a frame: inputs as stored, refraction = (0, 0, 0, alpha) as PrimaryRayGen leaves it.  scene as for reflection_pass, with
    `shadow` (light_rule.BruteForceShadows over the scene's triangles) and viewProj.  Returns dict: value, bound, decided, takes, total_internal, info."""
    assert mutate is None or mutate in MUTATIONS, mutate
    instance_id = np.asarray(instance_id); h, w = instance_id.shape
    refr = np.asarray(refraction, dtype=np.float64)
    takes = (instance_id >= 0) & (refr[..., 3] > EPSILON)                                                  # (G:23-27)
    py, px = np.nonzero(takes)
    n = len(px)
    origin = L.vec(np.asarray(position, dtype=np.float64)[takes][:, :3])
    v = L.vec(np.asarray(view, dtype=np.float64)[takes][:, :3]); nr = L.vec(np.asarray(normal, dtype=np.float64)[takes][:, :3])
    ids = instance_id[takes].astype(np.int64)
    eta = np.asarray([I["material"]["refractionFactor"] for I in scene["instances"]], dtype=np.float64)[ids]
    d, total, tir_und = hlsl_refract(v, nr, eta, mutate)                                                    # (G:34)
    alpha = F(refr[takes][:, 3])
    R = _resolve(scene, origin, d, alpha, ids, True, mutate)
    light, lwhy, have = _lights(scene, R, d, px, py, mutate != "glass_no_shadows", mutate)
    sky = scene["sky"]
    if S.described(sky):                                                                                    # SampleSky2D at the PIXEL's screen UV, not along the bent ray (G:112; E2-E6)
        sky = S.over_background([F(np.zeros(n)) for _ in range(3)], S.screen_colour(sky, sky["camera"], px, py, S.F16_STEP), sky.get("mutate"))
    vals, errs = [], []
    for c in range(3):
        rgb = L.where(have, L.mul(R["rgb"][c], L.add(R["ambient"][c], light[c])), R["rgb"][c])              # (G:108)
        rgb = L.add(rgb, L.add(L.mul(sky[c], R["a"]), R["transparent"][c]))                                # (G:112)
        out = L.add(F(refr[takes][:, c]), L.mul(rgb, alpha))                                                # (G:116)
        vals.append(out.v); errs.append(np.array(out.e))
    vals.append(alpha.v); errs.append(np.zeros(n))
    value, bound = _images(h, w, takes, vals, errs)
    bound[..., 3] = 0.0                                                                                      # alpha is kept: the same bytes
    value[~takes] = refr[~takes]
    why = dict(R["why"]); why.update({"light_" + k_: v_ for k_, v_ in lwhy.items()})
    why["total_internal"] = tir_und
    why["bound"] = np.isinf(bound[takes]).any(axis=-1)             # no finite bound (an error interval that reaches a pole): not claimed; a NaN is claimed, and wrong
    und = np.zeros(n, dtype=bool)
    for x in why.values():
        und |= x
    decided = np.ones((h, w), dtype=bool); decided[takes] = ~und

    def full(x, fill=0):
        a = np.full((h, w) + x.shape[1:], fill, dtype=x.dtype); a[takes] = x; return a
    return dict(value=value, bound=bound, decided=decided, takes=takes, total_internal=full(total),
                info=dict(hits=full(R["count"]), contributing=full(R["contributing"]), textured=full(R["textured"]), lit_surface=full(have), sky=full(R["a"].v > 0.0), undecided={k_: int(v_.sum()) for k_, v_ in why.items()}))


def compare(stored, value, bound, decided, takes):
    """(largest |stored - value| / bound over the decided pixels the pass takes, pixels at or outside the bound, mean ratio) of a stored image; a pixel the pass does not take
    must hold the value exactly (bound 0)."""
    dev = np.abs(np.asarray(stored, dtype=np.float64) - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(dev == 0.0, 0.0, dev / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio).max(axis=-1)
    ok = decided & takes
    rest = ~takes
    worst = float(ratio[ok].max()) if ok.any() else 0.0
    return worst, int((ratio[ok] >= 1.0).sum()) + int((ratio[rest] > 0.0).sum()), float(ratio[ok].mean()) if ok.any() else 0.0
