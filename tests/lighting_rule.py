"""Direct-light records of ray-query hits as a rule in numpy float64 (rules P1-P11).  TEST INFRASTRUCTURE.

`hit_light_kernel` (csrc/lighting.hip) joins what the library already computes elsewhere: the hit's position (surface.hip), its mapped normal and specular
texel (material.hip), the frame's light loop (shade.h) and the visibility walk (alpha_query.hip).  This module joins the rules those are held to and restates
nothing they state: position and side come from `surface_rule.surfaces`, normal and specular with their bounds from `material_rule.materials`, the interval
arithmetic, the admission estimate (`_intensity_simple`), one light's term (`_compute_light` at radius 0, without its shadow ray) and the constants from
`light_rule`, rule O2 from `alpha_rule.shadow_opaque`, the shadow alpha of a translucent caster from `material_rule` again.  What is stated here is the join:
every admitted light once at its centre (P4, P5), the shadow ray's window (P6), K5's subtraction over the candidates of the float64 shadow ray, P7's eye light,
and which records no float64 rule can decide.

A record is *undecided* when an admission (> 1e-6) lies within DECISION_K of its error, when a shadow ray passes a triangle's edge or the ends of its window
within the L7 margins (light_rule.triangle_test, K = 64) -- unless a shadow-opaque triangle is hit beyond doubt, which settles the ray whatever else it grazes --
when the alpha of a subtracting layer changes its texel, its cutout flag or its own decisions within the candidate's du, dv, when the visibility's interval holds
0 without being 0 (lightsBlocked could be either), when the hit's own normal or specular is undecided (A6, H8, H9), or when an error is not finite.
It imports nothing from oracle/ and nothing from the library.
"""
import numpy as np

import alpha_rule as AR
import light_rule as L
import material_rule as M
import surface_rule as S
from light_rule import F, U

VALID, BAD_HIT, BACK_FACE, UNLIT, TRUNCATED = 0x01, 0x02, 0x04, 0x08, 0x10
FLOOR = 2.0 ** -126          # the smallest normal float32: below it a stored value rounds in absolute steps
POINT_TEXEL_STEP = 2.0 ** -16          # a POINT-filtered alpha that moves by more than this within du, dv changed its texel (a UNORM8 step of a layer's alpha is >= 2^-8 x 0.05)

MUTATIONS = ("raydir_normalised", "point_radius_used", "offset_added", "tmin_no_bias", "ndotl_unclamped", "cap_scanned", "mask_zero_lit", "geometric_normal",
             "specular_map_ignored", "no_self_light", "cutouts_block", "shadow_by_solid_multiplier")
# the name light_rule gives the same mistake, where it has one
_LIGHT_RULE_NAME = {"point_radius_used": "radius_at_zero", "offset_added": "offset_added", "tmin_no_bias": "tmin_no_bias", "ndotl_unclamped": "ndotl_unclamped"}
_DUMMY_NOISE = np.full((512, 512, 4), 37, dtype=np.uint8)          # _compute_light reads a disc offset and multiplies it by radius 0; only "point_radius_used" sees it


# ---- P6: the shadow ray through any number of layers ----------------------------------------------------------------------------------------------------------

class ShadowWalks:
    """visibility(origin, direction (n, 3), tmin, tmax: F) of n shadow rays: K5 over the candidates brute force finds in float64, without culling.
    -> (F: the visibility and its bound, undecided [n], blocked [n]: 0 beyond doubt, walked [n]: the ray passed Q6)."""

    def __init__(self, data, levels, mutate=None, chunk=2048):
        self.data, self.levels, self.mutate, self.chunk = data, levels, mutate, chunk
        self.rt = S.raytraced_instances(data)
        self.opaque = AR.shadow_opaque(data, levels)
        self.groups = []
        for index in self.rt:
            inst = data.instances[index]
            mesh = data.meshes[inst.mesh]
            p = mesh.vertices["position"].astype(np.float64); p[:, 3] = 1.0
            world = (p @ np.asarray(inst.transform, dtype=np.float64))[:, :3]
            t = world[np.asarray(mesh.indices, dtype=np.int64)].reshape(-1, 3, 3)
            centre = 0.5 * (world.min(axis=0) + world.max(axis=0))
            self.groups.append((t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], centre, np.linalg.norm(world - centre, axis=1).max()))
        self.rays = 0

    def __call__(self, origin, direction, tmin, tmax):
        n = len(origin)
        self.rays += n
        walked = (tmin.v < tmax.v) & np.isfinite(origin).all(axis=1) & np.isfinite(direction).all(axis=1) & (direction != 0.0).any(axis=1)          # Q6
        window = np.abs(tmin.v - tmax.v) < L.DECISION_K * (tmin.e + tmax.e)                           # (whether it is walked at all)
        undecided = np.zeros(n, dtype=bool)
        stopped = np.zeros(n, dtype=bool)          # a shadow-opaque triangle hit beyond doubt
        grazed = np.zeros(n, dtype=bool)
        rows = []                                  # (ray, instance k, primitive, u, v, du, dv) of every translucent candidate hit beyond doubt
        with np.errstate(divide="ignore", invalid="ignore"):
            unit = direction / np.linalg.norm(direction, axis=1, keepdims=True)
        for k, (v0, e1, e2, centre, radius) in enumerate(self.groups):
            to_c = centre[None] - origin
            off = np.linalg.norm(to_c - (to_c * unit).sum(axis=1, keepdims=True) * unit, axis=1)
            near = np.nonzero(walked & (off <= radius * (1.0 + 2.0 ** -10)))[0]
            for a in range(0, len(near), self.chunk):
                i = near[a:a + self.chunk]
                u, v, t, du, dv, dt, _, ok = L.triangle_test(v0, e1, e2, origin[i], direction[i])
                w = 1.0 - u - v
                lo, hi = tmin.v[i, None], tmax.v[i, None]
                lo_e, hi_e = tmin.e[i, None] + dt, tmax.e[i, None] + dt
                hit = ok & (u > du) & (v > dv) & (w > du + dv) & (t > lo + lo_e) & (t < hi - hi_e)
                miss = ok & ((u < -du) | (v < -dv) | (w < -(du + dv)) | (t < lo - lo_e) | (t > hi + hi_e))
                grazed[i] |= (~hit & ~miss).any(axis=1)
                if self.opaque[k]:
                    stopped[i] |= hit.any(axis=1)
                else:
                    r, p = np.nonzero(hit)
                    rows += [(int(i[a_]), k, int(b_), u[a_, b_], v[a_, b_], du[a_, b_], dv[a_, b_]) for a_, b_ in zip(r, p)]
        total, bound, layers = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
        if rows:
            ray = np.array([r[0] for r in rows], dtype=np.int64)
            alpha, err, und = self._alphas(origin, direction, ray, rows)
            np.add.at(total, ray, alpha); np.add.at(bound, ray, err); np.add.at(layers, ray, 1)
            np.logical_or.at(stopped, ray, (alpha == 1.0) & (err == 0.0) & ~und)          # a layer that subtracts exactly 1 (H10's threshold) leaves max(v - 1, 0) = 0 whatever v was
            bad = np.zeros(n, dtype=bool); np.logical_or.at(bad, ray, und)
            undecided |= bad
        undecided |= grazed
        s = 1.0 - total
        e = bound + (layers + 1) * U
        vis = np.clip(s, 0.0, 1.0)
        err = np.maximum(np.clip(s + e, 0.0, 1.0) - vis, vis - np.clip(s - e, 0.0, 1.0))
        blocked = (s + e <= 0.0) & (layers > 0)
        undecided |= (layers > 0) & ~blocked & (s - e <= 0.0)          # 0 or just above it: lightsBlocked could be either
        undecided = (undecided & ~stopped) | window                    # (K6 ends the walk whatever else the ray grazes)
        vis = np.where(stopped, 0.0, vis); err = np.where(stopped, 0.0, err); blocked = blocked | stopped
        keep = walked | undecided
        return F(np.where(keep, vis, 1.0), np.where(keep, err, 0.0)), undecided, blocked & walked, walked

    def _point_texel(self, k):
        """Does the shadow alpha of instance k read a texel under the POINT filter?  (Then a move of u, v can change the texel, which no bound covers.)"""
        shader_id, filt = M.shader_of(self.data, self.data.instances[self.rt[k]])[:2]
        cc = M._combiner(shader_id)
        cycle = cc["c"][1] if (not cc["same"] and cc["alpha"]) else cc["c"][0]
        return filt == 0 and any(x in (5, 6) for x in cycle)

    def _alphas(self, origin, direction, ray, rows):
        """H10's shadow alpha of every candidate (K5: what the ray subtracts; 0 for a cutout) with its bound, and whether the candidate is undecided."""
        m = len(rows)
        rays = np.zeros((m, 8), dtype=np.float32)
        rays[:, 0:3] = origin[ray]; rays[:, 4:7] = direction[ray]; rays[:, 7] = np.inf
        uv = np.array([(r[3], r[4]) for r in rows]); duv = np.array([(r[5], r[6]) for r in rows])
        inst = np.array([r[1] for r in rows], dtype=np.uint32); prim = np.array([r[2] for r in rows], dtype=np.uint32)
        point = np.array([self._point_texel(k) for k in inst], dtype=bool)
        solid = self.mutate == "shadow_by_solid_multiplier"

        def at(su, sv):
            hits = np.zeros((m, 8), dtype=np.float32); hb = hits.view(np.uint32)
            hits[:, 1] = uv[:, 0] + su * duv[:, 0]; hits[:, 2] = uv[:, 1] + sv * duv[:, 1]
            hb[:, 3] = inst; hb[:, 4] = prim
            r = M.materials(self.data, self.levels, rays, hits, mutate="shadow_by_solid_multiplier" if solid else None)
            cut = (r["flags"] & M.SHADOW_CUTOUT) != 0
            a, e = r["shadow"][0][:, 0], r["shadow"][1][:, 0]
            if self.mutate == "cutouts_block":
                a = np.where(cut, 1.0, a)
            else:
                a = np.where(cut, 0.0, a); e = np.where(cut, 0.0, e)
            return a, e, cut, r["undecided"] | (r["kind"] != 2)
        a, e, cut, und = at(0.0, 0.0)
        spread = np.zeros(m)
        for su, sv in ((-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0)):          # the float32 u, v the device holds lie within du, dv of these
            a2, e2, cut2, und2 = at(su, sv)
            spread = np.maximum(spread, np.abs(a2 - a)); e = np.maximum(e, e2)
            und = und | und2 | (cut2 != cut)
        und = und | (point & (spread > POINT_TEXEL_STEP))
        return a, e + spread, und


# ---- P4, P5, P7 at given points -------------------------------------------------------------------------------------------------------------------------------

def _zeros3(n):
    return [F(np.zeros(n)) for _ in range(3)]


def core(st, mask_bits, self_light, lights, eye_diffuse, eye_specular, shadow, mutate=None):
    """The record's arithmetic for n points.  st: position, normal, specular, rayDirection as three F of n values each; ignoreNormalFactor, specularExponent,
    shadowRayBias [n].  mask_bits [n] uint32, self_light (n, 3); lights: dicts of the RT64_LIGHT fields; shadow: a ShadowWalks (or anything called like one).
    -> dict: direct, unshadowed, emitted (three F each), admitted, blocked [n] int, unlit, truncated [n] bool, why {kind: [n] bool}, partly [n] (a light seen
    through a layer), walks [n]."""
    assert mutate is None or mutate in MUTATIONS, mutate
    n = len(mask_bits)
    T = L._light_table(lights) if lights else None
    why = {k: np.zeros(n, dtype=bool) for k in ("admission", "shadow", "bound")}
    position, normal = st["position"], st["normal"]
    st_light = dict(st, px=np.zeros(n, dtype=np.int64), py=np.zeros(n, dtype=np.int64), bluenoise=_DUMMY_NOISE, frameCount=0, diSamples=0, checkShadows=False)
    mask = np.asarray(mask_bits, dtype=np.uint32)
    if mutate == "mask_zero_lit":
        mask = np.where(mask == 0, np.uint32(0xFFFFFFFF), mask)
    unlit = mask == 0
    count = np.zeros(n, dtype=np.int64); blocked = np.zeros(n, dtype=np.int64); walks = np.zeros(n, dtype=np.int64)
    last = np.full(n, -1, dtype=np.int64)          # index of the light admitted as the 16th
    partly = np.zeros(n, dtype=bool)
    direct, unshadowed = _zeros3(n), _zeros3(n)
    pending = []
    for l in range(len(lights)):
        if mutate == "cap_scanned" and l >= L.MAX_LIGHTS:
            break
        Ll = {k: np.broadcast_to(T[k][l], (n,) + T[k][l].shape) for k in L._LIGHT_FIELDS}
        scanned = ((mask & T["groupBits"][l]) != 0) & (count < L.MAX_LIGHTS)
        if not scanned.any():
            continue
        li, _ = L._intensity_simple(Ll, position, normal, st["ignoreNormalFactor"])                 # P4
        why["admission"] |= scanned & ~(np.abs(li.v - L.EPSILON) >= L.DECISION_K * li.e)
        admitted = scanned & (li.v > L.EPSILON)
        count += admitted
        last = np.where(admitted & (count == L.MAX_LIGHTS), l, last)
        if not admitted.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            term, _, _ = L._compute_light(Ll, st_light, admitted, _LIGHT_RULE_NAME.get(mutate))      # P5: radius 0, one sample, no shadow ray
            lp = L.vec(Ll["position"])
            distance = L.length3(L.sub3(position, lp))
            direction = L.normalize3(L.sub3(lp, position))
        tmin = L.add(L.RAY_MIN_DISTANCE, st["shadowRayBias"]) if mutate != "tmin_no_bias" else F(np.full(n, L.RAY_MIN_DISTANCE))          # P6
        tmax = L.sub(distance, Ll["shadowOffset"]) if mutate != "offset_added" else L.add(distance, Ll["shadowOffset"])
        i = np.nonzero(admitted)[0]
        pending.append((admitted, i, term, np.stack([c.v for c in position], axis=-1)[i], np.stack([c.v for c in direction], axis=-1)[i],
                        tmin.v[i], tmin.e[i], tmax.v[i], tmax.e[i]))
    if pending:          # every shadow ray of every record in one call, then the sums in list order
        cat = lambda k: np.concatenate([p[k] for p in pending])
        v, und, blk, walked = shadow(cat(3), cat(4), F(cat(5), cat(6)), F(cat(7), cat(8)))
        at = 0
        for admitted, i, term, *_ in pending:
            rows = slice(at, at + len(i)); at += len(i)
            vv, ve = np.ones(n), np.zeros(n); vv[i] = v.v[rows]; ve[i] = v.e[rows]
            vis = F(vv, ve)
            why["shadow"][i] |= und[rows]
            blocked[i] += blk[rows]; walks[i] += walked[rows]
            partly[i] |= ~und[rows] & (v.v[rows] > 0.0) & (v.v[rows] < 1.0)
            for c in range(3):
                unshadowed[c] = L.where(admitted, L.add(unshadowed[c], term[c]), unshadowed[c])
                direct[c] = L.where(admitted, L.add(direct[c], L.mul(term[c], vis)), direct[c])
    truncated = (last >= 0) & (last + 1 < len(lights))
    if mutate == "cap_scanned":
        truncated = np.full(n, len(lights) > L.MAX_LIGHTS) & ~unlit
    # P7: self light + eye light, with the direction as given
    ray_dir, spec = st["rayDirection"], st["specular"]
    eye_lambert = L.fmax(L.dot3(normal, L.neg3(ray_dir)), 0.0)
    eye_spec = L.power(L.fmax(L.saturate(L.dot3(L.reflect3(ray_dir, normal), L.neg3(ray_dir))), 0.0), st["specularExponent"])
    emitted = []
    for c in range(3):
        eye = L.add(L.mul(float(eye_diffuse[c]), eye_lambert), L.mul(float(eye_specular[c]), L.mul(spec[c], eye_spec)))
        emitted.append(L.add(F(np.zeros(n)) if mutate == "no_self_light" else F(np.asarray(self_light, dtype=np.float64)[:, c]), eye))
    for group in (direct, unshadowed, emitted):
        for c in group:
            why["bound"] |= ~np.isfinite(c.e) | ~np.isfinite(c.v)
    return {"direct": direct, "unshadowed": unshadowed, "emitted": emitted, "admitted": count, "blocked": blocked, "unlit": unlit, "truncated": truncated,
            "why": why, "partly": partly, "walks": walks}


def stored(fs):
    """Three F -> (value (n, 3), bound (n, 3)) of the float32 words a record holds: the propagated error, one rounding of the stored value, the float32 floor."""
    v = np.stack([c.v for c in fs], axis=-1); e = np.stack([np.broadcast_to(c.e, c.v.shape) for c in fs], axis=-1)
    return v, e + U * np.abs(v) + FLOOR


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------------

def scene_inputs(data):
    """What the rule reads of a scene besides its meshes and textures: the lights, the eye light, per ray-traced instance the five material fields."""
    lights = [dict(position=(l.position.x, l.position.y, l.position.z), diffuseColor=(l.diffuseColor.x, l.diffuseColor.y, l.diffuseColor.z),
                   attenuationRadius=l.attenuationRadius, pointRadius=l.pointRadius, specularColor=(l.specularColor.x, l.specularColor.y, l.specularColor.z),
                   shadowOffset=l.shadowOffset, attenuationExponent=l.attenuationExponent, groupBits=int(l.groupBits)) for l in data.lights]
    mats = []
    for index in S.raytraced_instances(data):
        m = data.instances[index].material
        mats.append(dict(lightGroupMaskBits=int(m.lightGroupMaskBits), ignoreNormalFactor=float(m.ignoreNormalFactor), specularExponent=float(m.specularExponent),
                         shadowRayBias=float(m.shadowRayBias), selfLight=(float(m.selfLight.x), float(m.selfLight.y), float(m.selfLight.z))))
    e = data.desc
    return dict(lights=lights, materials=mats, eye_diffuse=(e.eyeLightDiffuseColor.x, e.eyeLightDiffuseColor.y, e.eyeLightDiffuseColor.z),
                eye_specular=(e.eyeLightSpecularColor.x, e.eyeLightSpecularColor.y, e.eyeLightSpecularColor.z))


def lighting(data, levels, rays, hits, lods=None, mutate=None):
    """-> dict of per-record arrays: kind (0 miss, 1 bad hit, 2 real), direct / unshadowed / emitted as (value, bound) pairs of (N, 3) float64, flags, admitted,
    blocked, instance, primitive (int64), undecided (bool), and about the rule's own evaluation: in_shadow, partly, walks, why."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rays = np.asarray(rays, dtype=np.float32); hits = np.asarray(hits, dtype=np.float32)
    n = len(rays)
    surf = S.surfaces(data, rays, hits)
    mat = M.materials(data, levels, rays, hits, lods)
    real = surf["kind"] == 2
    i = np.nonzero(real)[0]
    m = len(i)
    inp = scene_inputs(data)
    ids = surf["instance"][i]
    field = lambda k: np.asarray([x[k] for x in inp["materials"]], dtype=np.float64)[ids] if m else np.zeros(0)
    rd = rays[i, 4:7].astype(np.float64)
    if mutate == "raydir_normalised":
        rd = rd / np.linalg.norm(rd, axis=1, keepdims=True)
    pick = lambda pair: [F(pair[0][i, c], pair[1][i, c]) for c in range(3)]
    normal = pick(mat["normal"])
    if mutate == "geometric_normal":
        sign = np.where(surf["back"][i], -1.0, 1.0)
        normal = [F(c.v * sign, c.e) for c in pick(surf["geometric"])]
    specular = [F(np.ones(m)) for _ in range(3)] if mutate == "specular_map_ignored" else pick(mat["specular"])
    st = {"position": pick(surf["position"]), "normal": normal, "specular": specular, "rayDirection": [F(rd[:, c]) for c in range(3)],
          "ignoreNormalFactor": field("ignoreNormalFactor"), "specularExponent": field("specularExponent"), "shadowRayBias": field("shadowRayBias")}
    mask_bits = np.asarray([x["lightGroupMaskBits"] for x in inp["materials"]], dtype=np.uint32)[ids] if m else np.zeros(0, dtype=np.uint32)
    self_light = np.asarray([x["selfLight"] for x in inp["materials"]], dtype=np.float64).reshape(-1, 3)[ids] if m else np.zeros((0, 3))
    res = core(st, mask_bits, self_light, inp["lights"], inp["eye_diffuse"], inp["eye_specular"], ShadowWalks(data, levels, mutate), mutate)

    out = {"kind": surf["kind"], "instance": surf["instance"], "primitive": surf["primitive"], "undecided": np.zeros(n, dtype=bool), "flags": np.zeros(n, dtype=np.int64),
           "admitted": np.zeros(n, dtype=np.int64), "blocked": np.zeros(n, dtype=np.int64), "in_shadow": np.zeros(n, dtype=bool), "partly": np.zeros(n, dtype=bool),
           "walks": np.zeros(n, dtype=np.int64)}
    for name in ("direct", "unshadowed", "emitted"):
        v, e = stored(res[name])
        out[name] = (np.zeros((n, 3)), np.zeros((n, 3)))
        out[name][0][i] = v; out[name][1][i] = e
    out["flags"][i] = VALID | np.where(surf["back"][i], BACK_FACE, 0) | np.where(res["unlit"], UNLIT, 0) | np.where(res["truncated"], TRUNCATED, 0)
    out["flags"][surf["kind"] == 1] = BAD_HIT
    out["admitted"][i] = res["admitted"]; out["blocked"][i] = res["blocked"]; out["partly"][i] = res["partly"]; out["walks"][i] = res["walks"]
    out["in_shadow"][i] = (res["blocked"] > 0) | res["partly"]
    why = dict(res["why"], surface=mat["undecided"][i] | surf["undecided"][i])
    und = np.zeros(m, dtype=bool)
    for w in why.values():
        und |= w
    out["undecided"][i] = und
    out["why"] = {k: int(w.sum()) for k, w in why.items()}
    return out


def at_gbuffer(data, levels, position, normal, specular, instance_id, camera, mutate=None):
    """P8: direct + emitted at a frame's stored G-buffer, as its RGBA16F DIRECT_LIGHT_RAW holds it when nothing is accumulated.  position, normal, specular:
    (H, W, >= 3) as stored; instance_id (H, W) int, < 0 for a miss; camera: light_rule.ray_direction's dict.  -> (value (H, W, 3), bound (H, W, 3), decided (H, W),
    info: the core's counts per pixel).  The bound is L8's: the propagated error and half an f16 step of the value."""
    lit = instance_id >= 0
    ids = instance_id[lit]
    n = len(ids)
    inp = scene_inputs(data)
    field = lambda k: np.asarray([x[k] for x in inp["materials"]], dtype=np.float64)[ids]
    rd = L.ray_direction(camera)[lit]
    rd_err = L.CAM_K * U * np.abs(rd).max(axis=-1)
    st = {"position": L.vec(np.asarray(position, dtype=np.float64)[lit]), "normal": L.vec(np.asarray(normal, dtype=np.float64)[lit]),
          "specular": L.vec(np.asarray(specular, dtype=np.float64)[lit]), "rayDirection": [F(rd[:, c], rd_err) for c in range(3)],
          "ignoreNormalFactor": field("ignoreNormalFactor"), "specularExponent": field("specularExponent"), "shadowRayBias": field("shadowRayBias")}
    mask_bits = np.asarray([x["lightGroupMaskBits"] for x in inp["materials"]], dtype=np.uint32)[ids]
    self_light = np.asarray([x["selfLight"] for x in inp["materials"]], dtype=np.float64).reshape(-1, 3)[ids]
    res = core(st, mask_bits, self_light, inp["lights"], inp["eye_diffuse"], inp["eye_specular"], ShadowWalks(data, levels, mutate), mutate)
    total = [L.add(a, b) for a, b in zip(res["direct"], res["emitted"])]
    v = np.stack([c.v for c in total], axis=-1); e = np.stack([c.e for c in total], axis=-1)
    h, w = instance_id.shape
    value, bound = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    value[lit] = v
    bound[lit] = e + np.maximum(L.F16_HALF_STEP * (np.abs(v) + e), L.F16_FLOOR)
    und = np.zeros(n, dtype=bool)
    for x in res["why"].values():
        und |= x
    decided = np.ones((h, w), dtype=bool); decided[lit] = ~und & np.isfinite(bound[lit]).all(axis=-1)
    info = {}
    for k in ("admitted", "blocked"):
        a = np.zeros((h, w), dtype=np.int64); a[lit] = res[k]; info[k] = a
    return value, bound, decided, info


def as_records(rule):
    """The rule's own values in RT64_RAY_LIGHTING's layout, (N, 16) float32, counters 0."""
    n = len(rule["kind"])
    rec = np.zeros((n, 16), dtype=np.float32); ri = rec.view(np.uint32)
    real = rule["kind"] == 2
    rec[:, 0:3] = rule["direct"][0]; rec[:, 4:7] = rule["unshadowed"][0]; rec[:, 8:11] = rule["emitted"][0]
    ri[:, 3] = rule["flags"]; ri[:, 7] = rule["admitted"]; ri[:, 11] = rule["blocked"]
    ri[:, 12] = np.where(real, rule["instance"], -1).astype(np.int64) & 0xFFFFFFFF
    ri[:, 13] = np.where(real, rule["primitive"], 0xFFFFFFFF)
    return rec


FIELDS = (("direct", slice(0, 3)), ("unshadowed", slice(4, 7)), ("emitted", slice(8, 11)))


def compare(rule, got, counters=False):
    """Per record: ratio |record - rule| / bound of direct, unshadowed, emitted (the largest over the components; a NaN counts as inf; 0 on undecided records), and
    whether flags, lightsAdmitted, lightsBlocked, instance and primitive are exactly the rule's.  An undecided record is held to VALID, instance and primitive
    and to finite floats.  Records that are not real hits must equal the miss / bad-hit record word for word.  counters: the device ran with count_traversal,
    so the last two words are free on records with a shadow walk; otherwise they are 0 everywhere."""
    got = np.asarray(got, dtype=np.float32); gi = got.view(np.uint32)
    want = as_records(rule); wi = want.view(np.uint32)
    real = rule["kind"] == 2
    decided = real & ~rule["undecided"]
    exact = (gi[:, 12] == wi[:, 12]) & (gi[:, 13] == wi[:, 13])
    exact &= np.where(decided, (gi[:, 3] == wi[:, 3]) & (gi[:, 7] == wi[:, 7]) & (gi[:, 11] == wi[:, 11]), (gi[:, 3] & (VALID | BAD_HIT)) == (wi[:, 3] & (VALID | BAD_HIT)))
    exact &= real | (gi == wi).all(axis=1)
    exact &= np.isfinite(got[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).all(axis=1)
    if counters:
        exact &= np.where(decided & (rule["walks"] == 0), (gi[:, 14] == 0) & (gi[:, 15] == 0), True)
    else:
        exact &= (gi[:, 14] == 0) & (gi[:, 15] == 0)
    ratios = {}
    for name, cols in FIELDS:
        v, e = rule[name]
        diff = np.abs(got[:, cols].astype(np.float64) - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff == 0.0, 0.0, diff / e)
        r = np.where(np.isnan(r), np.inf, r).max(axis=1)
        ratios[name] = np.where(decided, r, 0.0)
    return ratios, exact


def shares(rule):
    """Of the real hits: (in shadow, two or more lights admitted, a light seen through a layer, UNLIT, TRUNCATED, undecided)."""
    real = rule["kind"] == 2
    if not real.any():
        return (0.0,) * 6
    f = rule["flags"][real]
    return (float(rule["in_shadow"][real].mean()), float((rule["admitted"][real] >= 2).mean()), float(rule["partly"][real].mean()),
            float(((f & UNLIT) != 0).mean()), float(((f & TRUNCATED) != 0).mean()), float(rule["undecided"][real].mean()))


def report(name, rule, ratios, exact):
    """One line per case, laid out like profiles/material_rule_deviation.txt."""
    real = rule["kind"] == 2
    n = int(real.sum())
    parts = ["%-24s hits %5d of %5d" % (name, n, len(real))]
    for k, _ in FIELDS:
        r = ratios[k][real]
        parts.append("%s max %.3f mean %.4f" % (k, r.max() if n else 0.0, r.mean() if n else 0.0))
    bound = max(float(rule[k][1][real].max()) if n else 0.0 for k, _ in FIELDS)
    sh = shares(rule)
    parts.append("largest bound %.2e  undecided %.4f %s  shadow %.3f multi %.3f partly %.3f unlit %.3f truncated %.3f  inexact %d" %
                 (bound, sh[5], rule["why"], sh[0], sh[1], sh[2], sh[3], sh[4], int((~exact).sum())))
    return "  ".join(parts)
