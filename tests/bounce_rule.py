"""The frame's mirror and glass rays for ray-query hits as a rule in numpy float64 (rules R1-R12).  TEST INFRASTRUCTURE.

`hit_bounce_kernel` and `mirror_chain_kernel` (csrc/bounce.hip) join what the library computes elsewhere: the mapped shading normal of a hit (material.hip) and
the secondary rays of the reflection and refraction passes (passes.hip).  This module joins the rules those are held to and restates nothing they state: side
and the A4 position come from `surface_rule.surfaces`, the normal with its bound -- the texel box of a mapped normal included -- from `material_rule.materials`,
the interval arithmetic and `reflect3` from `light_rule` (the function `mirror_rule.reflection_pass` calls), `hlsl_refract` and `clamp` from `mirror_rule`.  What is
stated here is the join: the point on the ray (R2), the two directions from the direction AS GIVEN (R4, R5), the Fresnel amount of the hit's own instance (R6), the
flags, and which records no float64 rule can decide.

The bound of every output is the propagated float32 rounding of each operation (light_rule.F: half an ulp per sum and product, one ulp for sqrt, the documented
error of the device's log2 / exp2 for the fifth power), the normal's bound from material_rule, one rounding of the stored word and the float32 floor.
A record is *undecided* when one of three decisions lies inside its margin: back face or not (A6: |Ng . d| under DECISION_K times its error), k < 0 or not
(|k| under DECISION_K times its error), a POINT texel of the normal map (material_rule: the texel changes inside the UV's error) -- or when a bound is infinite.
It imports nothing from oracle/ and nothing from the library.
"""
import numpy as np

import light_rule as L
import material_rule as M
import mirror_rule as MR
import surface_rule as S
from light_rule import F, U

VALID, BAD_HIT, BACK_FACE, MIRROR, GLASS, TOTAL_INTERNAL, CONTINUED = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
EPSILON = L.EPSILON
T_MIN = L.RAY_MIN_DISTANCE
T_MAX = MR.RAY_MAX_DISTANCE
FLOOR = 2.0 ** -126          # the smallest normal float32: below it a stored value rounds in absolute steps
DECISION_K = L.DECISION_K
NORMAL_MAPPED = 0x08         # RT64_MATERIAL_NORMAL_MAPPED, as material_rule sets it

MUTATIONS = ("direction_normalised", "geometric_normal", "back_normal_not_turned", "no_depth_bias", "a4_position", "eta_inverted", "tir_ignored", "fresnel_no_floor",
             "fresnel_on_non_mirror", "tmin_zero")
_MATERIAL = ("reflectionFactor", "reflectionFresnelFactor", "refractionFactor", "depthBias")

reflect3 = L.reflect3          # d - 2 (N . d) N, the function mirror_rule.reflection_pass calls (M:39)
hlsl_refract = MR.hlsl_refract


def fresnel(normal, d, rf, ff, mutate=None):
    """rf + (1 - rf) clamp(1 + N . d, 1e-6, 1)^5 ff: mirror_rule._resolve's lines (M:19-23), with the factor of the instance handed in."""
    base = L.add(1.0, L.dot3(normal, d))
    ret = L.power(MR.clamp(base, EPSILON, 1.0), 5.0)
    if mutate == "fresnel_no_floor":                                       # pow of a negative base is not a number in HLSL
        ret = F(np.where(base.v < 0.0, np.nan, ret.v), ret.e)
    return L.add(rf, L.mul(L.mul(L.sub(1.0, rf), ret), ff))


def core(origin, d, t, normal, rf, ff, eta, bias, mutate=None):
    """R2, R4-R6 for n hits.  origin, d: three F each; t, rf, ff, eta, bias: exact float64 arrays of float32 numbers; normal: three F, already turned (R3).
    -> dict(position, reflected, refracted: three F; fresnel: F; mirror, glass, total: bool; tir_undecided: bool)"""
    dd = L.normalize3(d) if mutate == "direction_normalised" else d
    dist = L.sub(F(t), F(bias))                                            # the frame's hit record holds t - depthBias (its sort key) ...
    along = dist if mutate == "no_depth_bias" else L.add(dist, F(bias))    # ... and the resolve adds the bias back: two roundings, the point stays on the surface
    position = [L.add(origin[c], L.mul(d[c], along)) for c in range(3)]
    reflected = reflect3(dd, normal)
    refracted, total, tir_und = hlsl_refract(dd, normal, eta, mutate if mutate in ("eta_inverted", "tir_ignored") else None)
    mirror = rf > EPSILON
    fr = fresnel(normal, dd, rf, ff, mutate)
    if mutate != "fresnel_on_non_mirror":
        fr = L.where(mirror, fr, 0.0)
    return dict(position=position, reflected=reflected, refracted=refracted, fresnel=fr, mirror=mirror, glass=eta > EPSILON, total=total, tir_undecided=tir_und)


def stored(fs):
    """F's -> (value (n, k), bound (n, k)) of the float32 words a record holds: the propagated error, one rounding of the stored value, the float32 floor."""
    v = np.stack([c.v for c in fs], axis=-1); e = np.stack([np.broadcast_to(c.e, c.v.shape) for c in fs], axis=-1)
    return v, e + U * np.abs(v) + FLOOR


def material_table(data):
    """Per ray-traced instance the four material fields the rule reads, as the float32 numbers the device holds."""
    return {k: np.asarray([float(np.float32(getattr(data.instances[i].material, k))) for i in S.raytraced_instances(data)], dtype=np.float64) for k in _MATERIAL}


def bounces(data, levels, rays, hits, lods=None, mutate=None):
    """-> dict of per-record arrays: kind (0 miss, 1 bad hit, 2 real), position / reflected / refracted (value, bound) pairs of (N, 3), fresnel (N, 1),
    reflectionFactor / refractionFactor (float32), tmin (float32), flags, instance, primitive (int64), undecided (bool), mapped (bool), why."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rays = np.asarray(rays, dtype=np.float32); hits = np.asarray(hits, dtype=np.float32)
    n = len(rays)
    surf = S.surfaces(data, rays, hits)
    mat = M.materials(data, levels, rays, hits, lods)
    real = surf["kind"] == 2
    i = np.nonzero(real)[0]
    m = len(i)
    tab = material_table(data)
    ids = surf["instance"][i]
    field = lambda k: tab[k][ids] if m else np.zeros(0)
    pick = lambda pair: [F(pair[0][i, c], pair[1][i, c]) for c in range(3)]
    sign = np.where(surf["back"][i], -1.0, 1.0)
    normal = pick(mat["normal"])
    if mutate == "geometric_normal":
        normal = [F(c.v * sign, c.e) for c in pick(surf["geometric"])]
    if mutate == "back_normal_not_turned":
        normal = [F(c.v * sign, c.e) for c in normal]
    origin = [F(rays[i, c].astype(np.float64)) for c in range(3)]
    d = [F(rays[i, 4 + c].astype(np.float64)) for c in range(3)]
    res = core(origin, d, hits[i, 0].astype(np.float64), normal, field("reflectionFactor"), field("reflectionFresnelFactor"), field("refractionFactor"), field("depthBias"), mutate)
    if mutate == "a4_position":
        res["position"] = pick(surf["position"])

    out = {"kind": surf["kind"], "instance": surf["instance"], "primitive": surf["primitive"], "undecided": np.zeros(n, dtype=bool), "flags": np.zeros(n, dtype=np.int64),
           "mapped": np.zeros(n, dtype=bool), "reflectionFactor": np.zeros(n, dtype=np.float32), "refractionFactor": np.zeros(n, dtype=np.float32),
           "tmin": np.zeros(n, dtype=np.float32), "tmax": np.zeros(n, dtype=np.float32)}
    for name, k in (("position", 3), ("reflected", 3), ("refracted", 3), ("fresnel", 1)):
        v, e = stored(res[name] if k == 3 else [res[name]])
        out[name] = (np.zeros((n, k)), np.zeros((n, k)))
        out[name][0][i] = v; out[name][1][i] = e
    out["flags"][i] = (VALID | np.where(surf["back"][i], BACK_FACE, 0) | np.where(res["mirror"], MIRROR, 0) | np.where(res["glass"], GLASS, 0) |
                       np.where(res["total"], TOTAL_INTERNAL, 0))
    out["flags"][surf["kind"] == 1] = BAD_HIT
    out["mapped"][i] = (mat["flags"][i] & NORMAL_MAPPED) != 0
    out["reflectionFactor"][i] = field("reflectionFactor"); out["refractionFactor"][i] = field("refractionFactor")
    out["tmin"][i] = 0.0 if mutate == "tmin_zero" else T_MIN
    out["tmax"][i] = T_MAX
    bound_inf = np.zeros(m, dtype=bool)
    for name in ("position", "reflected", "refracted", "fresnel"):
        bound_inf |= np.isinf(out[name][1][i]).any(axis=1)          # no finite bound: not claimed; a NaN is claimed, and wrong
    why = {"side": surf["undecided"][i], "texel": mat["undecided"][i] & ~surf["undecided"][i], "total_internal": res["tir_undecided"], "bound": bound_inf}
    und = np.zeros(m, dtype=bool)
    for w in why.values():
        und |= w
    out["undecided"][i] = und
    out["why"] = {k: int(w.sum()) for k, w in why.items()}
    return out


def as_records(rule):
    """The rule's own values in the layout of the three outputs: (RT64_RAY_BOUNCEs, reflected RT64_RAYs, refracted RT64_RAYs), each (N, 8) float32, counters 0."""
    n = len(rule["kind"])
    real = rule["kind"] == 2
    rec = np.zeros((n, 8), dtype=np.float32); ri = rec.view(np.uint32)
    rec[:, 0] = rule["fresnel"][0][:, 0]; rec[:, 1] = rule["reflectionFactor"]; rec[:, 2] = rule["refractionFactor"]
    ri[:, 3] = rule["flags"]
    ri[:, 4] = np.where(real, rule["instance"], -1).astype(np.int64) & 0xFFFFFFFF
    ri[:, 5] = np.where(real, rule["primitive"], 0xFFFFFFFF)
    pair = []
    for name in ("reflected", "refracted"):
        r = np.zeros((n, 8), dtype=np.float32)
        r[:, 0:3] = rule["position"][0]; r[:, 3] = rule["tmin"]; r[:, 4:7] = rule[name][0]; r[:, 7] = rule["tmax"]
        pair.append(r)
    return rec, pair[0], pair[1]


FIELDS = ("fresnel", "position", "reflected", "refracted")


def compare(rule, got, counters=False):
    """got: (bounces, reflected, refracted), each (N, 8) float32.  Per record: ratio |got - rule| / bound of fresnel, position, reflected.direction and
    refracted.direction (the largest over the components; a NaN counts as inf; 0 on undecided records), and whether everything else is exactly the rule's: flags,
    instance, primitive, the two factors, tMin and tMax of both rays, and both origins the same bits.  An undecided record is held to VALID, MIRROR, GLASS,
    instance, primitive, the factors and to finite floats.  Records that are not real hits must equal the miss / bad-hit record word for word, both rays 32 zero
    bytes.  counters: the last two words are free (a walk made the records under count_traversal); otherwise they are 0."""
    rec, refl, refr = [np.ascontiguousarray(a, dtype=np.float32) for a in got]
    gi = rec.view(np.uint32)
    wrec, wrefl, wrefr = as_records(rule)
    wi = wrec.view(np.uint32)
    real = rule["kind"] == 2
    decided = real & ~rule["undecided"]
    keep = VALID | BAD_HIT | MIRROR | GLASS
    exact = (gi[:, 4] == wi[:, 4]) & (gi[:, 5] == wi[:, 5]) & (gi[:, 1] == wi[:, 1]) & (gi[:, 2] == wi[:, 2])
    exact &= np.where(decided, gi[:, 3] == wi[:, 3], (gi[:, 3] & keep) == (wi[:, 3] & keep))
    exact &= (refl.view(np.uint32)[:, 0:4] == refr.view(np.uint32)[:, 0:4]).all(axis=1)                     # one origin, one tMin
    for g, w in ((refl, wrefl), (refr, wrefr)):
        exact &= (g.view(np.uint32)[:, 3] == w.view(np.uint32)[:, 3]) & (g.view(np.uint32)[:, 7] == w.view(np.uint32)[:, 7])
        exact &= real | ~g.view(np.uint32).any(axis=1)
    exact &= real | ((gi[:, 0:6] == wi[:, 0:6]).all(axis=1))
    exact &= np.isfinite(rec[:, 0:3]).all(axis=1) & np.isfinite(refl).all(axis=1) & np.isfinite(refr).all(axis=1)
    if not counters:
        exact &= (gi[:, 6] == 0) & (gi[:, 7] == 0)
    ratios = {}
    for name, g in (("fresnel", rec[:, 0:1]), ("position", refl[:, 0:3]), ("reflected", refl[:, 4:7]), ("refracted", refr[:, 4:7])):
        v, e = rule[name]
        diff = np.abs(g.astype(np.float64) - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff == 0.0, 0.0, diff / e)
        r = np.where(np.isnan(r), np.inf, r).max(axis=1)
        ratios[name] = np.where(decided, r, 0.0)
    return ratios, exact


def shares(rule):
    """Of the real hits: (mirror, glass, total internal, back face, mapped normal, undecided)."""
    real = rule["kind"] == 2
    if not real.any():
        return (0.0,) * 6
    f = rule["flags"][real]
    return (float(((f & MIRROR) != 0).mean()), float(((f & GLASS) != 0).mean()), float(((f & TOTAL_INTERNAL) != 0).mean()), float(((f & BACK_FACE) != 0).mean()),
            float(rule["mapped"][real].mean()), float(rule["undecided"][real].mean()))


def report(name, rule, ratios, exact):
    """One line per case, laid out like profiles/lighting_rule_deviation.txt."""
    real = rule["kind"] == 2
    n = int(real.sum())
    parts = ["%-28s hits %5d of %5d" % (name, n, len(real))]
    for k in FIELDS:
        r = ratios[k][real]
        parts.append("%s max %.3f mean %.4f" % (k, r.max() if n else 0.0, r.mean() if n else 0.0))
    sh = shares(rule)
    parts.append("undecided %.4f %s  mirror %.3f glass %.3f total internal %.3f back %.3f mapped %.3f  inexact %d" %
                 (sh[5], rule["why"], sh[0], sh[1], sh[2], sh[3], sh[4], int((~exact).sum())))
    return "  ".join(parts)


def at_gbuffer(position, view, normal, instance_id, materials, half_step=0.0, normal_step=0.0):
    """R9: the rule's core at a frame's stored G-buffer.  position, view, normal: (H, W, >= 3) as stored; instance_id (H, W), < 0 for a miss; materials:
    material_table.  -> dict(lit, fresnel / reflected / refracted as (value, bound) over the lit pixels, total, tir_undecided).  The stored words are exact
    inputs at half_step = 0, as the reflection and refraction passes read them; half_step = light_rule.F16_HALF_STEP makes view and normal the unquantised values
    the primary resolve computed with, known to half an RGBA16F step; normal_step = mirror_rule.SNORM16_HALF_STEP adds what a record's unquantised normal differs
    by from the frame's, whose hit record holds the normal as SNORM16 before the image stores it."""
    lit = instance_id >= 0
    ids = instance_id[lit].astype(np.int64)
    v = L.vec(np.asarray(view, dtype=np.float64)[lit][:, :3]); nr = L.vec(np.asarray(normal, dtype=np.float64)[lit][:, :3])
    if half_step:
        v = [F(c.v, np.maximum(half_step * np.abs(c.v), L.F16_FLOOR)) for c in v]
        nr = [F(c.v, np.maximum(half_step * np.abs(c.v), L.F16_FLOOR) + normal_step) for c in nr]
    o = L.vec(np.asarray(position, dtype=np.float64)[lit][:, :3])
    zero = np.zeros(len(ids))
    res = core(o, v, zero, nr, materials["reflectionFactor"][ids], materials["reflectionFresnelFactor"][ids], materials["refractionFactor"][ids], zero)
    out = dict(lit=lit, total=res["total"], tir_undecided=res["tir_undecided"], mirror=res["mirror"])
    for name in ("reflected", "refracted"):
        out[name] = stored(res[name])
    out["fresnel"] = stored([res["fresnel"]])
    return out
