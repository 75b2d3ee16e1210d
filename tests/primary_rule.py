"""The primary resolve -- a pixel's hit list folded front to back into the G-buffer -- as a rule in numpy float64 (rules V1-V14).  TEST INFRASTRUCTURE.

`resolve_primary` / `store_primary` (csrc/passes.hip) and `pass_primary` (oracle/oracle_render.c) were written from the same HLSL by the same hand.  This module states
the operation a third time, from its meaning (PrimaryRayGen.hlsl:33-198, cited as (P:n); Fog.hlsli as (Fog:n)), in float64, with the `F` arithmetic of
tests/light_rule.py and the hit list, colours, normals and fog of tests/mirror_rule.py: every value carries a first-order bound on what a float32 evaluation may differ
by, every discrete decision is taken on the value, and a pixel whose decision has a margin below DECISION_K x the error of its two sides is reported undecided and held
only to what no decision touches (VIEW_DIRECTION).  It imports nothing from oracle/ and nothing from the library.

The rule's inputs are the scene as the host sent it and the cameras of this frame and the previous one -- never a stored image, except IMAGE_BACKGROUND for the
background term.  Its outputs are, per image, a value and a bound that includes the storage step (half an f16 step, half a UNORM8 step; float32 images one rounding).

The sky behind a pixel is tests/sky_rule.py's (E1-E8) where `scene["sky"]` is a sky description, else the one constant term of a scene whose sky texels are all equal.

Out of scope: normal and
specular maps and combiners other than mix-colour or TEX0 (H1-H12 hold them); the lod chosen by the primary ray differentials (textures have one level); hit lists past
16 entries (test_gpu_kbuffer.py); optNoise alpha; primary_spp > 1; what the next frame makes of the history guides normal[cur] and depth[cur] (tests/temporal_rule.py, rules N1-N8, reads them as DEPTH and -- on frames
without mirrors -- SHADING_NORMAL of the previous frame and holds the temporal accumulation of the GI pass to them); how a raster background
instance is drawn into IMAGE_BACKGROUND (tests/raster_rule.py, rules Z1-Z10, holds that; tests/test_gpu_raster.py compares it with the oracle's): this rule samples the
image as stored.  A scene has a constant sky term or a background image, not both; a described sky lies over the background by its alpha (E6).
"""
import math

import numpy as np

import light_rule as L
import mirror_rule as M
import sky_rule as S
from light_rule import F

EPSILON = L.EPSILON
DECISION_K = L.DECISION_K
APPLY_LIGHTS_MINIMUM_ALPHA = 0.5                    # Constants.hlsli:8
REACTIVE_CAP = float(np.float32(0.9))               # (P:194)
UNORM8_HALF_STEP = 0.5 / 255.0
JITTER_K = 4                                        # float32 roundings of a Halton value and of p + 0.5 + jitter, on top of CAM_K

MUTATIONS = ("state_last_hit", "state_from_unlit", "flow_x_not_negated", "flow_ignores_previous_transform", "flow_prev_matrix_current", "flow_not_in_pixels",
             "flow_miss_is_zero", "reproject_flag_ignored", "depth_without_bias", "fog_from_origin", "fresnel_direction_normalised", "reflect_alpha_summed",
             "lock_without_mirror_term", "lock_binary_with_upscaler", "reactive_unclamped", "reactive_from_sum", "glass_keeps_coverage", "transparent_light_per_hit",
             "transparent_light_unshadowed", "background_uv_at_pixel_centre", "jitter_not_in_uv", "alpha_is_remaining_coverage", "order_by_t")

IMAGES = ("position", "normal", "specular", "transparent", "flow", "reactive", "lock", "depth", "view", "reflection_a", "refraction_a")


# ---- V2: jitter ----------------------------------------------------------------------------------------------------------------------------------

def halton(index, base):
    """The radical inverse of `index` in `base` (tests/golden/kats.json pins the sequence)."""
    f, r, i = 1.0, 0.0, int(index)
    while i > 0:
        f /= base; r += f * (i % base); i //= base
    return r


def jitter(camera):
    """(V2) zero without an upscaler; with one Halton(frameCount mod phases + 1, 2 / 3) - 0.5."""
    if not camera.get("upscaler"):
        return 0.0, 0.0
    i = int(camera["frameCount"]) % int(camera["phases"]) + 1
    return halton(i, 2) - 0.5, halton(i, 3) - 0.5


def phase_count(display_width, render_width):
    return int(8.0 * (display_width / render_width) ** 2)


# ---- V13: matrices -------------------------------------------------------------------------------------------------------------------------------

def view_proj(cam):
    """view x projection in float64 from the float32 view matrix and perspective parameters (right-handed, row vectors; the aspect is the screen's)."""
    fov, zn, zf = float(np.float32(cam["fov"])), float(np.float32(cam["near"])), float(np.float32(cam["far"]))
    sy = 1.0 / math.tan(0.5 * fov); sx = sy / (cam["width"] / cam["height"]); rng = zf / (zn - zf)
    proj = np.zeros((4, 4)); proj[0, 0] = sx; proj[1, 1] = sy; proj[2, 2] = rng; proj[2, 3] = -1.0; proj[3, 2] = rng * zn
    return np.asarray(cam["view"], dtype=np.float32).astype(np.float64) @ proj


def _matrix_f(m):
    return [[F(np.float64(m[r][c]), L.CAM_K * L.U * abs(m[r][c])) for c in range(4)] for r in range(4)]


def _clip(Mf, p):
    return [L.add(L.add(L.add(L.mul(p[0], Mf[0][c]), L.mul(p[1], Mf[1][c])), L.mul(p[2], Mf[2][c])), Mf[3][c]) for c in range(4)]


def _screen(Mf, p):
    """(P:19-23) 0.5 + (clip.xy / clip.w) / 2 of exact points p (three F without an error of their own).  Returns (x, y, clip)."""
    clip = _clip(Mf, p)
    iw = L.rcp(clip[3])
    return L.add(0.5, L.mul(L.mul(clip[0], iw), 0.5)), L.add(0.5, L.mul(L.mul(clip[1], iw), 0.5)), clip


def _screen_gradient(m, p_v, axis):
    """d screen_axis / d p_c for c = 0, 1, 2 at the points p_v (n, 3) under the float64 matrix m."""
    clip = p_v @ m[:3] + m[3]
    w = clip[:, 3]
    return [0.5 * (m[c][axis] - clip[:, axis] / w * m[c][3]) / w for c in range(3)]


def flow_and_depth(pos, vflow, vp, pvp, size, mutate=None):
    """(V11) flow = (screen(viewProj, p) - screen(prevViewProj, p - vflow)) * size and depth = clip.z / clip.w under viewProj.  pos, vflow: three F each.  The error of the
    position moves both screen points together, so it is taken through the difference of their gradients (first order, as every bound here); the roundings of the
    evaluation are those of the F arithmetic on the values, with the matrices' float32 entries CAM_K roundings off.  Returns (fx, fy, depth)."""
    p = [F(c.v) for c in pos]; vf = [F(c.v) for c in vflow]
    Vf, Pf = _matrix_f(vp), _matrix_f(pvp)
    pp = L.sub3(p, vf)
    cx, cy, clip = _screen(Vf, p)
    qx, qy, _ = _screen(Pf, pp)
    p_v = np.stack([c.v for c in p], axis=-1); pp_v = np.stack([c.v for c in pp], axis=-1)
    out = []
    for axis, (a, b) in enumerate(((cx, qx), (cy, qy))):
        s = 1.0 if mutate == "flow_not_in_pixels" else float(size[axis])
        f = L.mul(L.sub(a, b), s)
        gc, gp = _screen_gradient(vp, p_v, axis), _screen_gradient(pvp, pp_v, axis)
        extra = sum(np.abs(gc[c] - gp[c]) * pos[c].e + np.abs(gp[c]) * vflow[c].e for c in range(3)) * abs(s)
        out.append(F(f.v, f.e + extra))
    depth = L.mul(clip[2], L.rcp(clip[3]))
    w = clip[3].v
    grad = sum(np.abs((vp[c][2] - depth.v * vp[c][3]) / w) * pos[c].e for c in range(3))
    return out[0], out[1], F(depth.v, depth.e + grad)


# ---- V14: the background term ----------------------------------------------------------------------------------------------------------------------

def background(image, px, py, jx, jy, size, mutate=None):
    """(V14, P:47-48) LINEAR / WRAP level-0 sample of the stored IMAGE_BACKGROUND (H, W, 4 bytes) at screenUV = (p + jitter) / size, WITHOUT the half pixel: at zero
    jitter the even blend of texels p - 1 and p.  The uv's float32 roundings (a sum, a quotient) move the sample through the texels' differences: tests/sampler_rule.py
    evaluates the corners of that box.  Returns three F."""
    import sampler_rule as SR
    half = 0.5 if mutate == "background_uv_at_pixel_centre" else 0.0
    if mutate == "jitter_not_in_uv":
        jx = jy = 0.0
    u, v = (px + half + jx) / size[0], (py + half + jy) / size[1]
    zero = np.zeros((len(u), 2))
    r = SR.sample_grad_bounds([np.asarray(image)], u, v, zero, zero, SR.LINEAR, SR.WRAP, SR.WRAP, 4.0 * L.U, 4.0 * L.U, 0.0, 8.0 * L.U)
    return [F(0.5 * (r["vmin"][:, c] + r["vmax"][:, c]), 0.5 * (r["vmax"][:, c] - r["vmin"][:, c]) + 8.0 * L.U) for c in range(3)]


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------------

def _fmax2(a, b):
    """max of two F."""
    v = np.maximum(a.v, b.v)
    return F(v, np.maximum(a.e, b.e))


def _object_flow(scene, tri, u, v, du, dv, mutate):
    """(V11) M q - M_prev q of hits: q the object-space point by barycentrics.  Exactly zero where the two transforms are the same matrix."""
    _, _, _, inst, prim = M.scene_triangles(scene)
    n = len(tri)
    out = [F(np.zeros(n)) for _ in range(3)]
    if mutate == "flow_ignores_previous_transform":
        return out
    for k, I in enumerate(scene["instances"]):
        here = inst[tri] == k
        T = np.asarray(I["transform"], dtype=np.float32).astype(np.float64); P = np.asarray(I["previousTransform"], dtype=np.float32).astype(np.float64)
        if not here.any() or np.array_equal(T, P):
            continue
        o = np.asarray(I["object_triangles"], dtype=np.float64).reshape(-1, 3, 3)[prim[tri[here]]]
        uu, vv = u[here][:, None], v[here][:, None]
        q = (1.0 - uu - vv) * o[:, 0] + uu * o[:, 1] + vv * o[:, 2]
        cur, prev = q @ T[:3, :3] + T[3, :3], q @ P[:3, :3] + P[3, :3]
        D = T[:3, :3] - P[:3, :3]
        spread = np.abs((o[:, 1] - o[:, 0]) @ D) * du[here][:, None] + np.abs((o[:, 2] - o[:, 0]) @ D) * dv[here][:, None]
        err = 8.0 * L.U * (np.abs(cur) + np.abs(prev) + np.abs(q).max(axis=1, keepdims=True) * (np.abs(T[:3, :3]).max() + np.abs(P[:3, :3]).max())) + spread
        for c in range(3):
            out[c] = M.put(out[c], here, F(cur[:, c] - prev[:, c], err[:, c]))
    return out


def _f16_bound(v, e):
    return e + np.maximum(L.F16_HALF_STEP * (np.abs(v) + e), L.F16_FLOOR)


def _unorm8_bound(v, e):
    """Half a UNORM8 step, and the two float32 roundings of x * 255 + 0.5 that decide a value on a step's edge (0.9 * 255 = 229.5 is one)."""
    return e + UNORM8_HALF_STEP + 2.0 * L.U * (np.abs(v) + e + 1.0 / 255.0)


def _stack(fs):
    return np.stack([c.v for c in fs], axis=-1), np.stack([np.broadcast_to(c.e, c.v.shape) for c in fs], axis=-1)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------------

def primary(scene, camera, mutate=None):
    """PrimaryRayGen for every pixel of a frame.

    scene: as mirror_rule's (instances in instance-id order with material -- here also `lockMask` --, world-space `triangles`, `normals`, `transform`, `cull`, `texture`;
    lights, ambientBase, ambientNoGI, sky, bluenoise, frameCount, diSamples, shadow) with, per instance, `previousTransform` and `object_triangles` (T, 3, 3).
    camera: view (4 x 4 float32), fov, near, far, width, height, frameCount, canReproject, previous (the previous frame's camera dict, or None when no frame was drawn
    before), upscaler (bool), phases, background (the stored IMAGE_BACKGROUND, (H, W, 4) bytes, or None when the scene has no background instance).
    Returns dict: images {name: (value, bound)} for IMAGES (|stored - value| <= bound is claimed at every decided pixel), diffuse_lo / diffuse_hi (H, W, 4 bytes the
    interval allows), id (H, W), lock_binary (bool), decided, lock_decided, first (tri, t, u, v and their bounds of the first list entry, count), info."""
    assert mutate is None or mutate in MUTATIONS, mutate
    w, h = int(camera["width"]), int(camera["height"])
    n = w * h
    jx, jy = jitter(camera)
    cam = dict(view=np.asarray(camera["view"], dtype=np.float32).astype(np.float64), fov=camera["fov"], near=camera["near"], far=camera["far"], width=w, height=h, jitter=(jx, jy))
    rd = L.ray_direction(cam).reshape(n, 3)                                                                 # (V1, P:35-39) not normalised
    rd_err = (L.CAM_K + JITTER_K) * L.U * np.abs(rd).max(axis=-1)
    direction = [F(rd[:, c], rd_err) for c in range(3)]
    o = np.linalg.inv(cam["view"])[3, :3]
    origin = [F(np.full(n, o[c]), L.CAM_K * L.U * np.abs(o).max()) for c in range(3)]
    py, px = np.divmod(np.arange(n), w)
    # (V13)
    vp = view_proj(camera)
    prev = camera.get("previous")
    reproject = (bool(camera["canReproject"]) or mutate == "reproject_flag_ignored") and prev is not None
    pvp = view_proj(prev) if (reproject and mutate != "flow_prev_matrix_current") else vp
    size = (w, h)
    fres_dir = L.normalize3(direction) if mutate == "fresnel_direction_normalised" else direction

    why = {k: np.zeros(n, dtype=bool) for k in ("hit", "order", "facing", "gate", "tie", "light_admission", "light_walk", "light_shadow", "light_bound")}
    hl = M.hit_lists(scene, np.tile(o, (n, 1)), rd, mutate=mutate)
    count = hl["count"]; why["hit"] |= ~hl["decided"]
    depth_max = int(count.max()) if n else 0
    assert depth_max <= M.MAX_HITS, "the hit list past 16 entries is out of scope"
    inst_of_tri = M.scene_triangles(scene)[3]
    mats = scene["instances"]
    tab = lambda key: np.asarray([m["material"][key] for m in mats], dtype=np.float64)
    zeros3 = lambda: [F(np.zeros(n)) for _ in range(3)]
    res_rgb, transparent, tl = zeros3(), zeros3(), zeros3()
    res_a, lock, refl_a, refr_a = F(np.ones(n)), F(np.zeros(n)), F(np.zeros(n)), F(np.zeros(n))
    st_pos, st_spec = zeros3(), zeros3()
    st_nrm = L.neg3(direction)                                                                              # (V12, P:75)
    st_id = np.full(n, -1, dtype=np.int64)
    tl_done = np.zeros(n, dtype=bool)
    contributing = np.zeros(n, dtype=np.int64); storing_hit = np.full(n, -1, dtype=np.int64); mirrors_n = np.zeros(n, dtype=np.int64)
    glass_px = np.zeros(n, dtype=bool); unlit_first = np.zeros(n, dtype=bool); tl_px = np.zeros(n, dtype=bool); fog_px = np.zeros(n, dtype=bool); textured = np.zeros(n, dtype=bool); tl_shadow = np.zeros(n, dtype=bool)
    # (V12, P:50-52, 81) the flow of the point origin + direction * 100000, depth 1
    far_pt = [F(o[c] + rd[:, c] * M.RAY_MAX_DISTANCE, L.U * (abs(o[c]) + 2.0 * np.abs(rd[:, c]) * M.RAY_MAX_DISTANCE) + rd_err * M.RAY_MAX_DISTANCE) for c in range(3)]
    fx, fy, _ = flow_and_depth(far_pt, zeros3(), vp, pvp, size, mutate)
    if mutate == "flow_miss_is_zero":
        fx, fy = F(np.zeros(n)), F(np.zeros(n))
    depth = F(np.ones(n))
    alive = count > 0
    ambient = [L.add(float(scene["ambientBase"][c]), float(scene["ambientNoGI"][c])) for c in range(3)]
    culls = np.asarray([bool(I["cull"]) for I in mats])
    masks = np.asarray([int(m_["material"]["lightGroupMaskBits"]) for m_ in mats], dtype=np.int64)
    for m in range(depth_max):
        has = alive & (count > m)
        if not has.any():
            break
        rows = np.nonzero(has)[0]
        g = lambda k: hl[k][rows, m]
        if depth_max > m + 1:                                                                             # (V3) as M3
            nxt = count[rows] > m + 1
            gap = np.where(nxt, hl["key"][rows, m + 1] - hl["key"][rows, m], np.inf)
            why["order"][rows] |= gap <= hl["key_e"][rows, m] + np.where(nxt, hl["key_e"][rows, m + 1], 0.0)
        tri = g("tri").astype(np.int64); inst = inst_of_tri[tri]
        culled = culls[inst]
        why["facing"][rows] |= ~culled & ~g("front_decided").astype(bool)
        k = len(rows)
        col, tie, tex_here = M.hit_colours(scene, tri, g("u"), g("v"), g("du"), g("dv"))                          # (V4)
        why["tie"][rows] |= tie
        h_alpha, tie = M.unorm8(tab("solidAlphaMultiplier")[inst]); why["tie"][rows] |= tie
        ra = M.take(res_a, rows)
        contrib = L.mul(ra, h_alpha)
        why["gate"][rows] |= np.abs(contrib.v - EPSILON) < DECISION_K * contrib.e
        passes = contrib.v >= EPSILON                                                                      # (V5, P:90)
        lk = M.take(lock, rows)
        lk = L.where(passes, L.add(lk, L.mul(F(tab("lockMask")[inst]), contrib)), lk)                      # (V6, P:94)
        uses = masks[inst] > 0
        apply = uses & (h_alpha.v > APPLY_LIGHTS_MINIMUM_ALPHA)                                            # (P:96-97)
        why["gate"][rows] |= uses & (np.abs(h_alpha.v - APPLY_LIGHTS_MINIMUM_ALPHA) < M.TIE)
        bias = tab("depthBias")[inst]
        key = L.sub(F(g("t"), g("dt")), bias)                                                              # the record's distance ...
        tt = key if mutate == "depth_without_bias" else L.add(key, bias)                                   # ... (t - bias) + bias (V4, P:98)
        d_r = [M.take(c, rows) for c in direction]; o_r = [M.take(c, rows) for c in origin]
        pos = L.add3(o_r, L.scale3(d_r, tt))
        nrm = M.hit_normals(scene, tri, g("u"), g("v"), g("du"), g("dv"), g("front").astype(bool) | culled)
        spec = [L.mul(F(np.asarray([m_["material"]["specularColor"][c] for m_ in mats], dtype=np.float64)[inst]), 1.0) for c in range(3)]
        store = np.zeros(k, dtype=bool)
        fog_on = tab("fogEnabled")[inst] != 0
        if fog_on.any():                                                                                   # (V7, P:107-111)
            fm, fo = np.where(fog_on, tab("fogMul")[inst], 1.0), np.where(fog_on, tab("fogOffset")[inst], 0.0)
            fa = M.fog_from_origin(pos, o_r, fm, fo) if mutate == "fog_from_origin" else M.fog_from_camera(pos, vp, fm, fo)
            fa = L.where(fog_on, fa, 0.0)
            fc = tab("fogColor")[inst]
            add_t = [L.mul(F(fc[:, c]), L.mul(fa, contrib)) for c in range(3)]
            contrib = L.where(fog_on, L.mul(contrib, L.sub(1.0, fa)), contrib)
        else:
            add_t = [F(np.zeros(k)) for _ in range(3)]
        rf = tab("reflectionFactor")[inst]
        mirrors = rf > EPSILON                                                                             # (V8, P:114-124)
        ra_refl = M.take(refl_a, rows)
        if mirrors.any():
            base = L.add(1.0, L.dot3(nrm, [M.take(c, rows) for c in fres_dir]))
            ret = L.power(M.clamp(base, EPSILON, 1.0), 5.0)
            fres = L.add(rf, L.mul(L.mul(L.sub(1.0, rf), ret), tab("reflectionFresnelFactor")[inst]))
            amount = L.mul(fres, contrib)
            on = passes & mirrors
            ra_refl = L.where(on, L.add(ra_refl, amount) if mutate == "reflect_alpha_summed" else amount, ra_refl)
            contrib = L.where(mirrors, L.mul(contrib, L.sub(1.0, fres)), contrib)
            if mutate != "lock_without_mirror_term":
                lk = L.where(on, L.add(lk, amount), lk)
            store |= mirrors
        self_light = tab("selfLight")[inst]
        # (V9) the one transparent-light draw, at the first hit that needs it
        needs = passes & uses & ~apply
        draw = needs & (~tl_done[rows] | (mutate == "transparent_light_per_hit"))
        tl_r = [M.take(c, rows) for c in tl]
        if draw.any():
            idx = np.nonzero(draw)[0]
            ids = inst[idx]
            st = {"position": [M.take(c, idx) for c in pos], "normal": [M.take(c, idx) for c in nrm], "specular": [M.take(c, idx) for c in spec],
                  "rayDirection": [M.take(c, idx) for c in d_r], "px": px[rows][idx], "py": py[rows][idx], "bluenoise": scene["bluenoise"],
                  "frameCount": int(scene["frameCount"]), "diSamples": int(scene["diSamples"]), "shadow": scene.get("shadow"),
                  "checkShadows": mutate != "transparent_light_unshadowed",
                  "ignoreNormalFactor": tab("ignoreNormalFactor")[ids], "specularExponent": tab("specularExponent")[ids], "shadowRayBias": tab("shadowRayBias")[ids]}
            res, lw, _, _, _, shadowed = L.light_loop(st, masks[ids].astype(np.uint32), scene["lights"], 1)
            for c in range(3):
                tl_r[c] = M.put(tl_r[c], draw, res[c])
            for kind, x in lw.items():
                why["light_" + kind][rows[idx]] |= x
            tl_done[rows[idx]] = True; tl_px[rows[idx]] = True; tl_shadow[rows[idx]] |= shadowed
        new_rgb, new_t = [], []
        for c in range(3):
            r_c, t_c = M.take(res_rgb[c], rows), M.take(transparent[c], rows)
            t_c = L.where(passes, L.add(t_c, add_t[c]), t_c)
            add_c = L.mul(col[c], contrib)                                                                 # (P:127)
            light_c = L.add(L.add(ambient[c], F(self_light[:, c])), tl_r[c])
            unlit_c = L.add(ambient[c], F(self_light[:, c]))
            t_lit = L.add(t_c, L.mul(add_c, light_c)); t_unlit = L.add(t_c, L.mul(add_c, unlit_c))
            new_rgb.append(L.where(passes & apply, L.add(r_c, add_c), r_c))
            new_t.append(L.where(passes & needs, t_lit, L.where(passes & ~uses, t_unlit, t_c)))
        store |= apply
        if mutate == "state_from_unlit":
            store |= ~uses
        ra_new = L.where(passes, L.mul(ra, L.sub(1.0, h_alpha)), ra)                                       # (V10, P:150)
        glass = passes & (tab("refractionFactor")[inst] > EPSILON)                                         # (P:153-157)
        rr = L.where(glass, ra_new, M.take(refr_a, rows))
        if mutate != "glass_keeps_coverage":
            ra_new = L.where(glass, 0.0, ra_new)
        store |= glass
        storing = passes & store & ((st_id[rows] < 0) | (mutate == "state_last_hit"))                      # (V11, P:160)
        vflow = _object_flow(scene, tri, g("u"), g("v"), g("du"), g("dv"), mutate)
        hfx, hfy, hdepth = flow_and_depth(pos, vflow, vp, pvp, size, mutate)
        # write back
        for c in range(3):
            res_rgb[c] = M.put(res_rgb[c], has, new_rgb[c]); transparent[c] = M.put(transparent[c], has, new_t[c]); tl[c] = M.put(tl[c], has, tl_r[c])
            st_pos[c] = M.put(st_pos[c], has, L.where(storing, pos[c], M.take(st_pos[c], rows)))
            st_nrm[c] = M.put(st_nrm[c], has, L.where(storing, nrm[c], M.take(st_nrm[c], rows)))
            st_spec[c] = M.put(st_spec[c], has, L.where(storing, spec[c], M.take(st_spec[c], rows)))
        fx = M.put(fx, has, L.where(storing, hfx, M.take(fx, rows))); fy = M.put(fy, has, L.where(storing, hfy, M.take(fy, rows)))
        depth = M.put(depth, has, L.where(storing, hdepth, M.take(depth, rows)))
        storing_hit[rows] = np.where(storing & (storing_hit[rows] < 0), m, storing_hit[rows])
        unlit_first[rows] |= passes & ~store & (st_id[rows] < 0) & (contributing[rows] == 0)
        st_id[rows] = np.where(storing, inst, st_id[rows])
        contributing[rows] += passes; mirrors_n[rows] += passes & mirrors; glass_px[rows] |= glass; fog_px[rows] |= passes & fog_on; textured[rows] |= passes & tex_here
        lock = M.put(lock, has, lk); refl_a = M.put(refl_a, has, ra_refl); refr_a = M.put(refr_a, has, rr)
        res_a = M.put(res_a, has, ra_new)
        why["gate"][rows] |= passes & (ra_new.v > 0.0) & (np.abs(ra_new.v - EPSILON) < DECISION_K * ra_new.e)
        stop = np.zeros(n, dtype=bool); stop[rows] = ra_new.v <= EPSILON                                   # (V5, P:174)
        alive = alive & ~stop

    # (V14)
    peak = _fmax2(transparent[0], _fmax2(transparent[1], transparent[2]))
    if mutate == "reactive_from_sum":
        peak = L.add(L.add(transparent[0], transparent[1]), transparent[2])
    reactive = peak if mutate == "reactive_unclamped" else M.fmin(peak, REACTIVE_CAP)
    reactive = M.fmin(reactive, 1.0)                                                                      # UNORM8 saturates
    bg = scene["sky"]                                                                                     # bg = lerp(background, sky.rgb, sky.a): sky.a is 1 (one opaque texel value) or no sky
    if S.described(bg):                                                                                   # ... or a sky description: SampleSky2D at the pixel's screen UV (tests/sky_rule.py, E2-E6)
        back = [F(np.zeros(n)) for _ in range(3)]
        if camera.get("background") is not None:
            back = background(camera["background"], px.astype(np.float64), py.astype(np.float64), jx, jy, size, mutate)
        colour = S.screen_colour(bg, dict(view=cam["view"], width=w, height=h, jitter=(jx, jy)), px, py)
        bg = S.over_background(back, colour, bg.get("mutate"))
    elif camera.get("background") is not None:
        assert all(float(np.abs(c.v).max()) == 0.0 for c in bg), "a sky term or a background image, not both"
        bg = background(camera["background"], px.astype(np.float64), py.astype(np.float64), jx, jy, size, mutate)
    rgb = [L.add(res_rgb[c], L.mul(bg[c], res_a)) for c in range(3)]
    alpha = res_a if mutate == "alpha_is_remaining_coverage" else L.sub(1.0, res_a)
    binary = (not camera.get("upscaler")) or mutate == "lock_binary_with_upscaler"
    lock_und = np.zeros(n, dtype=bool)
    if binary:
        lock_und = np.abs(lock.v - 0.5) < DECISION_K * lock.e
        lock_out = F((lock.v >= 0.5).astype(np.float64))
    else:
        lock_out = M.fmin(lock, 1.0)
    has_hit = st_id >= 0

    def img(fs, bound):
        v, e = _stack(fs)
        return v.reshape(h, w, -1), bound(v, e).reshape(h, w, -1)
    f32 = lambda v, e: e + L.U * np.abs(v)
    images = {"position": img(st_pos, f32), "normal": img(st_nrm, _f16_bound), "specular": img(st_spec, _f16_bound), "transparent": img(transparent, _f16_bound),
              "flow": img([fx, fy] if mutate == "flow_x_not_negated" else [L.neg(fx), fy], _f16_bound), "reactive": img([reactive], _unorm8_bound),
              "lock": img([lock_out], (lambda v, e: e) if binary else _unorm8_bound), "depth": img([depth], f32), "view": img(direction, _f16_bound),
              "reflection_a": img([refl_a], _f16_bound), "refraction_a": img([refr_a], _f16_bound)}
    dv, de = _stack(rgb + [alpha])
    dv, de = np.clip(dv, 0.0, 1.0), de + 2.0 * L.U
    lo = np.clip(np.ceil(np.clip(dv - de, 0.0, 1.0) * 255.0 - 0.5 - 1e-9), 0, 255).reshape(h, w, 4)
    hi = np.clip(np.floor(np.clip(dv + de, 0.0, 1.0) * 255.0 + 0.5 + 1e-9), 0, 255).reshape(h, w, 4)
    why["bound"] = np.zeros(n, dtype=bool)
    for v, b in images.values():
        why["bound"] |= ~np.isfinite(b).all(axis=-1).reshape(n)
    why["bound"] |= ~np.isfinite(de).all(axis=-1)                                                          # DIFFUSE under a sky colour that is claimed nowhere (E7)
    und = np.zeros(n, dtype=bool)
    for x in why.values():
        und |= x
    sh = lambda x: x.reshape(h, w)
    first = {k: sh(hl[k][:, 0]) for k in ("tri", "t", "u", "v", "dt", "du", "dv")}
    first["count"] = sh(count)
    return dict(images=images, diffuse_lo=lo, diffuse_hi=hi, id=sh(st_id), lock_binary=binary, decided=sh(~und), lock_decided=sh(~und & ~lock_und), first=first,
                info=dict(hits=sh(count), contributing=sh(contributing), has_hit=sh(has_hit), storing_hit=sh(storing_hit), mirrors=sh(mirrors_n), glass=sh(glass_px),
                          unlit_first=sh(unlit_first), transparent_light=sh(tl_px), transparent_light_shadowed=sh(tl_shadow), fog=sh(fog_px), textured=sh(textured), background=sh((res_a.v > 0.0) & (camera.get("background") is not None)), lock=sh(lock.v), reactive=sh(peak.v), coverage=sh(1.0 - res_a.v),
                          flow=np.stack([fx.v, fy.v], axis=-1).reshape(h, w, 2), jitter=(jx, jy),
                          undecided=dict({k_: int(v_.sum()) for k_, v_ in why.items()}, lock_step=int((lock_und & ~und).sum()))))
