"""The colour a ray brings back as a rule in numpy float64 (rules W1-W12).  TEST INFRASTRUCTURE.

`ray_radiance_kernel` (csrc/radiance.hip) joins the list walk, the layers' colours, the light loop and the sky.  This module states what it must answer a second
time, from what the other rules already state, with the `F` arithmetic of tests/light_rule.py: every value carries a first-order bound on what a float32
evaluation may differ by, every discrete decision is taken on the value, and a ray whose decision has a margin below DECISION_K x the error of its sides is
reported undecided instead of guessed.  It imports nothing from the library and nothing from oracle/:
  the list        layers_rule.lists over enumerated candidates (the caller enumerates them), its UNORM8 alpha steps and its undecided rays (list order, T2 / T5);
  the colour      material_rule.materials at the ray's lod, each channel through the frame's UNORM8 store -- a tie within the colour's bound is undecided;
  the light       lighting_rule.lighting at the lit layer's hit: facing, admission and every shadow walk are its decisions, its `why` is carried;
  the sky         sky_rule.plane_colour / over_background along the direction as given, over no background;
  the fog         mirror_rule.fog_from_origin / fog_from_camera.
The decisions of this module's own: the two 1e-6 gates (w >= 1e-6, rem <= 1e-6).

W5's position is origin + direction x reach, reach = (t - depthBias) + depthBias: t and depthBias are float32 numbers the record and the material hold, so reach is
restated in float32 exactly and carries no error; the product and the sum are the F arithmetic's.
"""
import numpy as np

import layers_rule as LR
import light_rule as L
import lighting_rule as P
import material_rule as M
import mirror_rule as MR
import sky_rule as S
import surface_rule as SF
from light_rule import F, U

EPSILON = L.EPSILON
DECISION_K = L.DECISION_K
FLOOR = P.FLOOR
VALID, COVERED, BAD_HIT, LIT, FOGGED, TRUNCATED = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
FLAG_UNSHADOWED, FLAG_FOG_FROM_CAMERA = 0x100, 0x200

MUTATIONS = ("lit_first_layer", "lit_only_lit_layers", "eye_light_added", "fog_after_colour", "fog_from_camera_default", "unlit_without_ambient", "colour_unquantised",
             "sky_unweighted", "skipped_layer_scales_rem", "shadowed_under_unshadowed")
# fake_envmap_uv takes two atan2 of ratios of the direction's components: a positive factor on the direction changes neither, so the sky by the normalised direction
# is the same sky (tests/test_radiance_rule.py pins that on values) and cannot be told from the rule.
EQUIVALENT = ("sky_by_normalised_direction",)
FIELDS = (("radiance", slice(0, 3)), ("surface", slice(4, 7)), ("transparent", slice(8, 11)), ("light", slice(12, 15)))


def sky_of(data, width, height):
    """The description tests/sky_rule.py reads, or None for a scene without a sky texture (RGBA8, level 0; no frame of these cases makes the tiled copy)."""
    if data.sky is None:
        return None
    e = data.desc
    v3 = lambda x: (float(x.x), float(x.y), float(x.z))
    return dict(texels=np.asarray(data.textures[data.sky].data), multiplier=v3(e.skyDiffuseMultiplier), hsl=v3(e.skyHSLModifier), yawOffset=float(e.skyYawOffset),
                camera=dict(view=np.asarray(data.view, dtype=np.float32), width=width, height=height, jitter=(0.0, 0.0)), tiled=False, mutate=None)


def view_proj(data, width, height):
    """view x projection, row vectors, as tests/mirror_cases.py builds it for the camera fog."""
    sy = 1.0 / np.tan(0.5 * float(data.fov)); sx = sy / (width / height); rng = float(data.far) / (float(data.near) - float(data.far))
    proj = np.zeros((4, 4)); proj[0, 0] = sx; proj[1, 1] = sy; proj[2, 2] = rng; proj[2, 3] = -1.0; proj[3, 2] = rng * float(data.near)
    return np.asarray(data.view, dtype=np.float32).astype(np.float64) @ proj


def _quantise(v, e):
    """The frame's UNORM8 store of values in [0, 1] with bound e: (k / 255 as F, tie).  k = floor(255 v + 0.5), 0 unless v > 0, 255 from 1 on."""
    v = np.asarray(v, dtype=np.float64)
    scaled = np.clip(v, 0.0, 1.0) * 255.0 + 0.5
    k = np.clip(np.floor(scaled), 0, 255)
    margin = np.minimum(scaled - np.floor(scaled), np.floor(scaled) + 1.0 - scaled)
    tie = (margin < 255.0 * DECISION_K * e + 4 * 256 * U) & (v > 0.0) & (v < 1.0)
    q = k / 255.0
    return F(q, np.where((k == 0) | (k == 255), 0.0, 2.0 * U * q)), tie


def _take(f, idx):
    return F(f.v[idx], f.e[idx])


def _put(dst, idx, src):
    v = dst.v.copy(); e = np.array(dst.e, dtype=np.float64); v[idx] = src.v; e[idx] = src.e
    return F(v, e)


def radiance(data, levels, rays, cand, lods=None, flags=0, sky=None, viewproj=None, max_layers=16, oracle_scene=None, mutate=None):
    """-> dict: radiance / surface / transparent / light as (value, bound) pairs of (N, 3) -- the bound is the propagated error, one rounding of the stored float32
    and its floor --, transmittance (value, bound) [N], lit [N] (-1: none), layers [N], flags [N], undecided [N], why {kind: count}, and the rule's own counts:
    fogged, unlit_last (the last contributor has lightGroupMaskBits 0), shaded_by_walk (a light is partly or fully blocked at the lit layer)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rays = np.asarray(rays, dtype=np.float32)
    n = len(rays)
    lods = np.zeros(n, dtype=np.float32) if lods is None else np.asarray(lods, dtype=np.float32)
    lr = LR.lists(data, levels, rays, cand, lods, oracle_scene=oracle_scene)
    index, hits = cand
    mat = M.materials(data, levels, rays[index], hits, lods[index])
    inst_of = hits.view(np.int32)[:, 3].astype(np.int64)
    rt = SF.raytraced_instances(data)
    mats = [data.instances[i].material for i in rt]
    f32 = lambda x: float(np.float32(x))
    tab = lambda f: np.array([f(m) for m in mats], dtype=np.float64)
    mask = np.array([int(m.lightGroupMaskBits) for m in mats], dtype=np.int64)
    self_light = tab(lambda m: (f32(m.selfLight.x), f32(m.selfLight.y), f32(m.selfLight.z))).reshape(-1, 3)
    fog_on = np.array([int(m.fogEnabled) for m in mats], dtype=np.int64)
    fog_colour = tab(lambda m: (f32(m.fogColor.x), f32(m.fogColor.y), f32(m.fogColor.z))).reshape(-1, 3)
    fog_mul, fog_offset = tab(lambda m: f32(m.fogMul)), tab(lambda m: f32(m.fogOffset))
    bias32 = np.array([np.float32(m.depthBias) for m in mats], dtype=np.float32)
    e = data.desc
    ambient = [L.add(f32(getattr(e.ambientBaseColor, c)), f32(getattr(e.ambientNoGIColor, c))) for c in "xyz"]

    rows = np.full((n, max_layers), -1, dtype=np.int64)
    for k, r in enumerate(lr["rows"]):
        m = min(len(r), max_layers)
        rows[k, :m] = r[:m]
    why = {k: np.zeros(n, dtype=bool) for k in ("list", "alpha", "colour", "gate", "fog", "light", "bound")}
    why["list"] |= lr["undecided"]
    origin, direction = L.vec(rays[:, 0:3].astype(np.float64)), L.vec(rays[:, 4:7].astype(np.float64))
    rem = F(np.ones(n))
    surface = [F(np.zeros(n)) for _ in range(3)]; transparent = [F(np.zeros(n)) for _ in range(3)]
    lit = np.full(n, -1, dtype=np.int64); lit_row = np.full(n, -1, dtype=np.int64)
    shaded = np.zeros(n, dtype=np.int64); out_flags = np.where(lr["valid"], VALID, 0).astype(np.int64)
    alive = lr["valid"].copy()
    from_camera = bool(flags & FLAG_FOG_FROM_CAMERA) != (mutate == "fog_from_camera_default")
    for l in range(max_layers):
        idx = np.nonzero(alive & (rows[:, l] >= 0))[0]
        alive &= rows[:, l] >= 0                                                        # the list's end
        if not len(idx):
            break
        r = rows[idx, l]; inst = inst_of[r]
        why["alpha"][idx] |= lr["und_alpha"][r]
        q = lr["quantum"][r] / 255.0
        a = F(q, np.where((q == 0.0) | (q == 1.0), 0.0, 2.0 * U * q))
        col, tie = [], np.zeros(len(idx), dtype=bool)
        for c in range(3):
            if mutate == "colour_unquantised":
                col.append(F(mat["color"][0][r, c], mat["color"][1][r, c]))
            else:
                x, t_ = _quantise(mat["color"][0][r, c], mat["color"][1][r, c]); col.append(x); tie |= t_
        rm = _take(rem, idx)
        w = L.mul(rm, a)
        near = np.abs(w.v - EPSILON) < DECISION_K * w.e + 2 * U * EPSILON
        passes = w.v >= EPSILON                                                          # W5
        why["gate"][idx] |= near
        why["colour"][idx] |= tie & passes
        why["colour"][idx] |= mat["undecided"][r]
        reach = ((hits[r, 0] - bias32[inst]) + bias32[inst]).astype(np.float64)          # float32, exactly
        o_r, d_r = [_take(c, idx) for c in origin], [_take(c, idx) for c in direction]
        pos = L.add3(o_r, L.scale3(d_r, F(reach)))
        fogged = passes & (fog_on[inst] != 0)
        w_f, add_t = w, [F(np.zeros(len(idx))) for _ in range(3)]
        if fogged.any():
            fm, fo = np.where(fogged, fog_mul[inst], 1.0), np.where(fogged, fog_offset[inst], 0.0)
            fa = MR.fog_from_camera(pos, viewproj, fm, fo) if from_camera else MR.fog_from_origin(pos, o_r, fm, fo)
            fa = L.where(fogged, fa, 0.0)
            why["fog"][idx] |= fogged & ~np.isfinite(fa.e)
            add_t = [L.mul(F(fog_colour[inst, c]), L.mul(fa, w)) for c in range(3)]
            w_f = L.where(fogged, L.mul(w, L.sub(1.0, fa)), w)
        w_c = w if mutate == "fog_after_colour" else w_f                                 # (the mutation adds the colour before the fog takes its share)
        lit_layer = mask[inst] > 0
        for c in range(3):
            s_c, t_c = _take(surface[c], idx), _take(transparent[c], idx)
            t_c = L.where(fogged, L.add(t_c, add_t[c]), t_c)
            term = L.mul(col[c], w_c)
            unlit = term if mutate == "unlit_without_ambient" else L.mul(term, L.add(ambient[c], F(self_light[inst, c])))
            surface[c] = _put(surface[c], idx, L.where(passes & lit_layer, L.add(s_c, term), s_c))
            transparent[c] = _put(transparent[c], idx, L.where(passes & ~lit_layer, L.add(t_c, unlit), t_c))
        keeps = passes
        if mutate == "lit_first_layer":
            keeps = passes & (lit[idx] < 0)
        elif mutate == "lit_only_lit_layers":
            keeps = passes & lit_layer
        lit[idx] = np.where(keeps, l, lit[idx]); lit_row[idx] = np.where(keeps, r, lit_row[idx])
        shaded[idx] += passes
        out_flags[idx] |= np.where(fogged, FOGGED, 0)
        scales = passes | (mutate == "skipped_layer_scales_rem")
        rm_new = L.where(scales, L.mul(rm, L.sub(1.0, a)), rm)
        rem = _put(rem, idx, rm_new)
        why["gate"][idx] |= scales & (rm_new.v != 0.0) & (np.abs(rm_new.v - EPSILON) < DECISION_K * rm_new.e + 2 * U * EPSILON)
        stop = rm_new.v <= EPSILON
        out_flags[idx] |= np.where(stop, COVERED, 0)
        alive[idx[stop]] = False
    # W6: the light at the lit layer
    has = lit >= 0
    at = np.zeros((n, 8), dtype=np.float32); ab = at.view(np.uint32)
    at[:, 0] = np.inf; ab[:, 3] = 0xFFFFFFFF; ab[:, 4] = 0xFFFFFFFF
    at[has] = hits[lit_row[has]]
    lg = P.lighting(data, levels, rays, at, lods)
    unshadowed = bool(flags & FLAG_UNSHADOWED) and mutate != "shadowed_under_unshadowed"
    term = lg["unshadowed"] if unshadowed else lg["direct"]
    why["light"] |= has & lg["undecided"]
    k_lit = np.where(has, inst_of[np.maximum(lit_row, 0)], 0)
    light = []
    for c in range(3):
        d = F(term[0][:, c], term[1][:, c])
        if mutate == "eye_light_added":
            d = L.add(d, L.sub(F(lg["emitted"][0][:, c], lg["emitted"][1][:, c]), F(self_light[k_lit, c])))
        light.append(L.where(has, L.add(ambient[c], L.add(d, F(self_light[k_lit, c]))), 0.0))
    out_flags |= np.where(has, LIT, 0) | np.where(has & ((lg["flags"] & P.TRUNCATED) != 0), TRUNCATED, 0)
    # W1 / W7
    if sky is not None:
        colour = S.plane_colour(sky, direction)
        skyc = S.over_background([F(np.zeros(n)) for _ in range(3)], colour)
    else:
        skyc = [F(np.zeros(n)) for _ in range(3)]
    res = {}
    rad = []
    for c in range(3):
        x = L.where(has, L.mul(surface[c], light[c]), surface[c])
        if mutate == "sky_unweighted":
            back = skyc[c]
        else:          # a ray with no coverage left does not see the sky, whatever bound its colour has
            gone = (rem.v == 0.0) & (rem.e == 0.0)
            with np.errstate(invalid="ignore"):
                back = L.where(gone, 0.0, L.mul(F(np.where(gone, 0.0, skyc[c].v), np.where(gone, 0.0, skyc[c].e)), rem))
        x = L.add(x, L.add(back, transparent[c]))
        rad.append(L.where(lr["valid"], x, 0.0))
    for name, fs in (("radiance", rad), ("surface", surface), ("transparent", transparent), ("light", light)):
        res[name] = P.stored(fs)
        why["bound"] |= ~np.isfinite(res[name][1]).all(axis=1)
    res["transmittance"] = (rem.v.copy(), np.array(rem.e) + U * np.abs(rem.v))
    und = np.zeros(n, dtype=bool)
    for x in why.values():
        und |= x
    und &= lr["valid"]
    last_unlit = has & (mask[k_lit] == 0)
    res.update(lit=lit, layers=shaded, flags=out_flags, undecided=und, valid=lr["valid"], why={k: int(x.sum()) for k, x in why.items()},
               fogged=(out_flags & FOGGED) != 0, unlit_last=last_unlit, shaded_by_walk=has & lg["in_shadow"], lists=lr, sky=P.stored(skyc))
    return res


def compare(rule, got):
    """got: (N, 16) float32 RT64_RAY_RADIANCEs -> (ratios {field: [N] largest |got - value| / bound, 0 on undecided rays}, exact [N]: transmittance within its bound and
    litLayer, layers and flags equal, True on undecided rays)."""
    got = np.ascontiguousarray(got, dtype=np.float32); gb = got.view(np.uint32)
    und = rule["undecided"]

    def ratio(g, v, e):
        d = np.abs(g.astype(np.float64) - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d == 0.0, 0.0, d / e)
        return np.where(np.isnan(r), np.inf, r)
    ratios = {name: np.where(und, 0.0, ratio(got[:, sl], *rule[name]).max(axis=1)) for name, sl in FIELDS}
    ratios["transmittance"] = np.where(und, 0.0, ratio(got[:, 7], *rule["transmittance"]))
    exact = (gb[:, 11].view(np.int32) == rule["lit"]) & (gb[:, 15] == rule["layers"]) & (gb[:, 3] == rule["flags"])
    return ratios, exact | und


def differs(a, b):
    """[N] bool: the rays two evaluations of the rule answer differently beyond their bounds, among those both decide."""
    out = (a["lit"] != b["lit"]) | (a["layers"] != b["layers"]) | (a["flags"] != b["flags"])
    for name, _ in FIELDS:
        out |= (np.abs(a[name][0] - b[name][0]) > a[name][1] + b[name][1]).any(axis=1)
    out |= np.abs(a["transmittance"][0] - b["transmittance"][0]) > a["transmittance"][1] + b["transmittance"][1]
    return out & ~a["undecided"] & ~b["undecided"]
