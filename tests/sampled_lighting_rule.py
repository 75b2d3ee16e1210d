"""Sampled direct-light records of ray-query hits as a rule in numpy float64 (rules J1-J11).  TEST INFRASTRUCTURE.

`hit_sampled_light_kernel` (csrc/sampled_lighting.hip) joins what the library already computes elsewhere, and so does this module: the shaded point with its
bounds comes from `surface_rule.surfaces` and `material_rule.materials` exactly as `lighting_rule.lighting` takes it; the draws, the disc, one light's term, the
interval arithmetic and the brute-force shadow ray are `light_rule.light_loop` and `light_rule.BruteForceShadows` (rules L2-L7), called once per group of records
that share `key.frame` because the loop takes one frame count; `emitted` is `lighting_rule.core` without lights (P7).  What is stated here is the join and the four
things no other rule has: the `drawn` mask (L3's walk once more, on values, returning slots), `unshadowed` (the same loop with every shadow term 1), the
overrides (J4) and J8's integer noise factor -- `tests/test_oracle_kats.py` shows the hash and tests/golden/kats.json pins it.

Shadow casters are opaque or noise casters whose alpha is exactly 1 before the factor (sampled_lighting_cases builds no other): a record whose factor is 0 is
lit as if its noise casters were not there, one whose factor is 1 as if they were opaque.  A record is *undecided* under L7's conditions -- an admission, a
comparison of a walk or a shadow ray within its margin, an error that is not finite -- or when the hit's own normal or specular is undecided.
It imports nothing from oracle/ and nothing from the library.
"""
import numpy as np

import light_cases as LC
import light_rule as L
import lighting_rule as P
import material_rule as M
import surface_rule as S
from light_rule import F

VALID, BAD_HIT, BACK_FACE, UNLIT, TRUNCATED = P.VALID, P.BAD_HIT, P.BACK_FACE, P.UNLIT, P.TRUNCATED

MUTATIONS = ("key_frame_ignored", "xy_swapped", "mod64_dropped", "noise_frame_of_view", "noise_row_of_64", "overrides_ignored", "invprob_always", "not_zeroed",
             "sample_slot_up", "radius_at_zero", "unshadowed_shadowed", "drawn_by_index")
# the name light_rule gives the same mistake, where it has one
_LIGHT_RULE_NAME = {"mod64_dropped": "bn_no_xmod", "invprob_always": "invprob_always", "not_zeroed": "not_zeroed", "sample_slot_up": "sample_slot_up",
                    "radius_at_zero": "radius_at_zero"}


# ---- J8: the factor of a noise caster ---------------------------------------------------------------------------------------------------------------------------

def init_rand(v0, v1, backoff=16):
    """Random.hlsli:14-26 on uint32 arrays (the hash of tests/test_oracle_kats.py::_tea)."""
    v0 = np.asarray(v0, dtype=np.uint64) & 0xFFFFFFFF; v1 = np.asarray(v1, dtype=np.uint64) & 0xFFFFFFFF
    m = np.uint64(0xFFFFFFFF); s0 = np.uint64(0)
    for _ in range(backoff):
        s0 = (s0 + np.uint64(0x9e3779b9)) & m
        v0 = (v0 + ((((v1 << np.uint64(4)) & m) + np.uint64(0xa341316c)) ^ (v1 + s0) ^ ((v1 >> np.uint64(5)) + np.uint64(0xc8013ea4)))) & m
        v1 = (v1 + ((((v0 << np.uint64(4)) & m) + np.uint64(0xad90777d)) ^ (v0 + s0) ^ ((v0 >> np.uint64(5)) + np.uint64(0x7e95761e)))) & m
    return v0


def noise_factor(x, y, frame, width):
    """rint(next_rand(init_rand(x + y * width, frame, 16))): 0 or 1, an integer decision with no margin (24 bits of an LCG step over 2^24; 0.5 rounds to even)."""
    seed = init_rand((np.asarray(x, dtype=np.uint64) + np.asarray(y, dtype=np.uint64) * np.uint64(width)) & np.uint64(0xFFFFFFFF), frame)
    s = (np.uint64(1664525) * seed + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
    return np.rint((s & np.uint64(0x00FFFFFF)).astype(np.float64) / float(0x01000000)).astype(np.int64)


# ---- J6: which slots the draws take ---------------------------------------------------------------------------------------------------------------------------------

def drawn_mask(intensity, index, count, noise, max_lights, zeroing=True, by_index=False):
    """L3's walk on values.  intensity (n, 16) float64 and index (n, 16) int: the candidate columns; count [n]; noise (draws, n): blue_noise(x, y, frame + s).red.
    -> [n] uint32: bit k for candidate slot k drawn, bit 16 + k for slot k reached again after it was zeroed."""
    n = len(count)
    col = np.array(intensity, dtype=np.float64)
    remaining = np.zeros(n)
    for k in range(16):          # in slot order, as the scan adds them up
        remaining = np.where(k < count, remaining + col[:, k], remaining)
    drawn = np.zeros(n, dtype=np.int64)
    rows = np.arange(n)
    draws = np.minimum(count, int(max_lights))
    single = (count == 1) & (int(max_lights) >= 1)
    for s in range(int(draws.max()) if n else 0):
        active = s < draws
        r = noise[s] * remaining
        chosen = np.zeros(n, dtype=np.int64)
        running = col[:, 0].copy()
        walking = active & ~single
        for _ in range(15):
            step = walking & (chosen < count - 1) & (r >= running)
            chosen = chosen + step
            running = np.where(step, running + col[rows, chosen], running)
            walking = step
            if not step.any():
                break
        c_int = col[rows, chosen]
        bit = np.where(by_index, index[rows, chosen], chosen)
        again = (drawn >> bit) & 1
        drawn = np.where(active, drawn | np.where(again == 1, np.int64(0x10000) << bit, np.int64(1) << bit), drawn)
        if zeroing:
            col[rows[active & ~single], chosen[active & ~single]] = 0.0
        remaining = np.where(active & ~single, remaining - c_int, remaining)
    return drawn


def _candidates(st, mask_bits, lights):
    """P4's scan as lighting_rule.core does it: -> (intensity (n, 16), index (n, 16), count [n], truncated [n])."""
    n = len(mask_bits)
    T = L._light_table(lights) if lights else None
    count = np.zeros(n, dtype=np.int64); last = np.full(n, -1, dtype=np.int64)
    inten = np.zeros((n, 16)); index = np.zeros((n, 16), dtype=np.int64)
    for l in range(len(lights)):
        Ll = {k: np.broadcast_to(T[k][l], (n,) + T[k][l].shape) for k in L._LIGHT_FIELDS}
        scanned = ((mask_bits & T["groupBits"][l]) != 0) & (count < L.MAX_LIGHTS)
        if not scanned.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            li, _ = L._intensity_simple(Ll, st["position"], st["normal"], st["ignoreNormalFactor"])
        admitted = scanned & (li.v > L.EPSILON)
        i = np.nonzero(admitted)[0]
        inten[i, count[i]] = li.v[i]; index[i, count[i]] = l
        count += admitted
        last = np.where(admitted & (count == L.MAX_LIGHTS), l, last)
    return inten, index, count, (last >= 0) & (last + 1 < len(lights))


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------------------------------------

def _take(fs, i):
    return [F(c.v[i], np.broadcast_to(c.e, c.v.shape)[i]) for c in fs]


def noise_casters(data):
    """[k] bool per ray-traced instance: does its shader have the noise option?"""
    return [M._combiner(M.shader_of(data, data.instances[index])[0])["noise"] for index in S.raytraced_instances(data)]


def core(data, st, mask_bits, self_light, kx, ky, kf, frame, max_lights=-1, di_samples=-1, mutate=None):
    """The record's arithmetic for m points.  st: position, normal, specular, rayDirection as three F of m values each; ignoreNormalFactor, specularExponent,
    shadowRayBias [m].  kx, ky, kf [m]: the keys; frame: dict(width, height, frameCount, maxLights, diSamples) of the view's last drawn frame.
    -> dict: direct, unshadowed, emitted (three F each), admitted, drawn, draws, factor [m] int, unlit, truncated, in_shadow [m] bool, why {kind: [m] bool}."""
    assert mutate is None or mutate in MUTATIONS, mutate
    m = len(mask_bits)
    width = int(frame["width"])
    kx, ky, kf = (np.asarray(a).astype(np.int64) & 0xFFFFFFFF for a in (kx, ky, kf))
    if mutate == "overrides_ignored" or max_lights < 0:
        max_lights = frame["maxLights"]
    if mutate == "overrides_ignored" or di_samples < 0:
        di_samples = frame["diSamples"]
    if mutate == "xy_swapped":
        kx, ky = ky, kx
    if mutate == "key_frame_ignored":
        kf = np.full(m, int(frame["frameCount"]), dtype=np.int64)
    inp = P.scene_inputs(data)

    # J8: one integer per key; the casters a record's shadow rays see
    factor = noise_factor(kx, ky, np.full(m, int(frame["frameCount"])) if mutate == "noise_frame_of_view" else kf, 64 if mutate == "noise_row_of_64" else width)
    tris = LC.rule_inputs(data)["triangles"]
    noisy = noise_casters(data)
    shadows = {1: L.BruteForceShadows(tris)}
    shadows[0] = L.BruteForceShadows([t for t, nz in zip(tris, noisy) if not nz]) if any(noisy) else shadows[1]

    direct, unshadowed = [[F(np.zeros(m)) for _ in range(3)] for _ in range(2)]
    why = {k: np.zeros(m, dtype=bool) for k in ("admission", "walk", "shadow", "bound")}
    admitted = np.zeros(m, dtype=np.int64); draws = np.zeros(m, dtype=np.int64); in_shadow = np.zeros(m, dtype=bool)
    inner = _LIGHT_RULE_NAME.get(mutate)
    groups = {}
    for r in range(m):
        groups.setdefault((int(kf[r]), int(factor[r]) if any(noisy) else 1), []).append(r)
    for (f, fac), rows in sorted(groups.items()):          # light_loop takes one frame count (and one set of casters)
        g = np.asarray(rows, dtype=np.int64)
        sub = {k: (_take(v, g) if isinstance(v, list) else v[g]) for k, v in st.items()}
        sub.update(px=kx[g], py=ky[g], bluenoise=data.bluenoise, frameCount=f, diSamples=int(di_samples), shadow=shadows[fac])
        with np.errstate(divide="ignore", invalid="ignore"):
            lit, w, count, drew, _, shd = L.light_loop(sub, mask_bits[g], inp["lights"], max_lights, mutate=inner)
            bare = lit if mutate == "unshadowed_shadowed" else L.light_loop(dict(sub, checkShadows=False), mask_bits[g], inp["lights"], max_lights, mutate=inner)[0]
        for c in range(3):
            for dst, src in ((direct, lit), (unshadowed, bare)):
                v = dst[c].v.copy(); e = np.array(dst[c].e); v[g] = src[c].v; e[g] = src[c].e
                dst[c] = F(v, e)
        for k in ("admission", "walk", "shadow"):
            why[k][g] |= w[k]
        admitted[g] = count; draws[g] = drew; in_shadow[g] = shd

    # J6's mask, from the same candidates
    inten, index, count, truncated = _candidates(st, mask_bits, inp["lights"])
    assert np.array_equal(count, admitted)
    most = int(min(max(int(max_lights), 0), 16))
    noise = np.zeros((max(most, 1), m))
    for s in range(most):
        for f in np.unique(kf):
            g = np.nonzero(kf == f)[0]
            noise[s, g] = L.blue_noise(data.bluenoise, kx[g], ky[g], int(f) + s, 0, mutate != "mod64_dropped").v
    drawn = drawn_mask(inten, index, count, noise, max_lights, zeroing=mutate != "not_zeroed", by_index=mutate == "drawn_by_index")

    with np.errstate(divide="ignore", invalid="ignore"):
        emitted = P.core(st, mask_bits, self_light, [], inp["eye_diffuse"], inp["eye_specular"], None)["emitted"]          # J9
    unlit = mask_bits == 0
    return {"direct": direct, "unshadowed": unshadowed, "emitted": emitted, "admitted": admitted, "drawn": drawn, "draws": draws, "factor": factor, "unlit": unlit,
            "truncated": truncated & ~unlit, "in_shadow": in_shadow, "why": why}


def sampled(data, levels, rays, hits, keys, frame, lods=None, max_lights=-1, di_samples=-1, mutate=None):
    """-> dict of per-record arrays: kind (0 miss, 1 bad hit, 2 real), direct / unshadowed / emitted as (value, bound) pairs of (N, 3) float64, flags, admitted,
    drawn, instance, primitive (int64), undecided (bool), and about the rule's own evaluation: in_shadow, draws, factor, why.
    keys: (N, 4) uint32, or None for J3's default; frame: dict(width, height, frameCount, maxLights, diSamples) of the view's last drawn frame."""
    rays = np.asarray(rays, dtype=np.float32); hits = np.asarray(hits, dtype=np.float32)
    n = len(rays)
    if keys is None:
        assert n <= int(frame["width"]) * int(frame["height"])
        keys = np.stack([np.arange(n) % int(frame["width"]), np.arange(n) // int(frame["width"]), np.full(n, frame["frameCount"]), np.zeros(n, dtype=np.int64)], axis=1)
    keys = np.asarray(keys).astype(np.int64) & 0xFFFFFFFF
    surf = S.surfaces(data, rays, hits)
    mat = M.materials(data, levels, rays, hits, lods)
    real = surf["kind"] == 2
    i = np.nonzero(real)[0]
    m = len(i)
    inp = P.scene_inputs(data)
    ids = surf["instance"][i]
    field = lambda k: np.asarray([x[k] for x in inp["materials"]], dtype=np.float64)[ids] if m else np.zeros(0)
    rd = rays[i, 4:7].astype(np.float64)
    pick = lambda pair: [F(pair[0][i, c], pair[1][i, c]) for c in range(3)]
    st = {"position": pick(surf["position"]), "normal": pick(mat["normal"]), "specular": pick(mat["specular"]), "rayDirection": [F(rd[:, c]) for c in range(3)],
          "ignoreNormalFactor": field("ignoreNormalFactor"), "specularExponent": field("specularExponent"), "shadowRayBias": field("shadowRayBias")}
    mask_bits = np.asarray([x["lightGroupMaskBits"] for x in inp["materials"]], dtype=np.uint32)[ids] if m else np.zeros(0, dtype=np.uint32)
    self_light = np.asarray([x["selfLight"] for x in inp["materials"]], dtype=np.float64).reshape(-1, 3)[ids] if m else np.zeros((0, 3))
    res = core(data, st, mask_bits, self_light, keys[i, 0], keys[i, 1], keys[i, 2], frame, max_lights, di_samples, mutate)

    out = {"kind": surf["kind"], "instance": surf["instance"], "primitive": surf["primitive"], "undecided": np.zeros(n, dtype=bool), "flags": np.zeros(n, dtype=np.int64),
           "admitted": np.zeros(n, dtype=np.int64), "drawn": np.zeros(n, dtype=np.int64), "in_shadow": np.zeros(n, dtype=bool), "draws": np.zeros(n, dtype=np.int64),
           "factor": np.zeros(n, dtype=np.int64)}
    why = dict(res["why"])
    for name in ("direct", "unshadowed", "emitted"):
        v, e = P.stored(res[name])
        why["bound"] = why["bound"] | ~np.isfinite(v).all(axis=1) | ~np.isfinite(e).all(axis=1)
        out[name] = (np.zeros((n, 3)), np.zeros((n, 3)))
        out[name][0][i] = v; out[name][1][i] = e
    out["flags"][i] = VALID | np.where(surf["back"][i], BACK_FACE, 0) | np.where(res["unlit"], UNLIT, 0) | np.where(res["truncated"], TRUNCATED, 0)
    out["flags"][surf["kind"] == 1] = BAD_HIT
    for k in ("admitted", "drawn", "in_shadow", "draws", "factor"):
        out[k][i] = res[k]
    why["surface"] = mat["undecided"][i] | surf["undecided"][i]
    und = np.zeros(m, dtype=bool)
    for w in why.values():
        und |= w
    out["undecided"][i] = und
    out["why"] = {k: int(w.sum()) for k, w in why.items()}
    return out


def at_gbuffer(data, position, normal, specular, instance_id, camera, frame, max_lights=-1, di_samples=-1, mutate=None):
    """J10: direct + emitted at a frame's stored G-buffer with keys (px, py, frameCount), as its RGBA16F DIRECT_LIGHT_RAW holds it when nothing is accumulated.
    position, normal, specular: (H, W, >= 3) as stored; instance_id (H, W) int, < 0 for a miss; camera: light_rule.ray_direction's dict.
    -> (value (H, W, 3), bound (H, W, 3): L8's, decided (H, W), drawn (H, W))."""
    lit = instance_id >= 0
    ids = instance_id[lit]
    py, px = np.nonzero(lit)
    n = len(ids)
    inp = P.scene_inputs(data)
    field = lambda k: np.asarray([x[k] for x in inp["materials"]], dtype=np.float64)[ids]
    rd = L.ray_direction(camera)[lit]
    rd_err = L.CAM_K * L.U * np.abs(rd).max(axis=-1)
    st = {"position": L.vec(np.asarray(position, dtype=np.float64)[lit]), "normal": L.vec(np.asarray(normal, dtype=np.float64)[lit]),
          "specular": L.vec(np.asarray(specular, dtype=np.float64)[lit]), "rayDirection": [F(rd[:, c], rd_err) for c in range(3)],
          "ignoreNormalFactor": field("ignoreNormalFactor"), "specularExponent": field("specularExponent"), "shadowRayBias": field("shadowRayBias")}
    mask_bits = np.asarray([x["lightGroupMaskBits"] for x in inp["materials"]], dtype=np.uint32)[ids]
    self_light = np.asarray([x["selfLight"] for x in inp["materials"]], dtype=np.float64).reshape(-1, 3)[ids]
    res = core(data, st, mask_bits, self_light, px, py, np.full(n, int(frame["frameCount"])), frame, max_lights, di_samples, mutate)
    total = [L.add(a, b) for a, b in zip(res["direct"], res["emitted"])]
    v = np.stack([c.v for c in total], axis=-1); e = np.stack([c.e for c in total], axis=-1)
    h, w = instance_id.shape
    value, bound, drawn = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w), dtype=np.int64)
    value[lit] = v
    bound[lit] = e + np.maximum(L.F16_HALF_STEP * (np.abs(v) + e), L.F16_FLOOR)
    drawn[lit] = res["drawn"]
    und = np.zeros(n, dtype=bool)
    for x in res["why"].values():
        und |= x
    decided = np.ones((h, w), dtype=bool); decided[lit] = ~und & np.isfinite(bound[lit]).all(axis=-1)
    return value, bound, decided, drawn


def as_records(rule):
    """The rule's own values in RT64_RAY_SAMPLED_LIGHTING's layout, (N, 16) float32, counters 0."""
    n = len(rule["kind"])
    rec = np.zeros((n, 16), dtype=np.float32); ri = rec.view(np.uint32)
    real = rule["kind"] == 2
    rec[:, 0:3] = rule["direct"][0]; rec[:, 4:7] = rule["unshadowed"][0]; rec[:, 8:11] = rule["emitted"][0]
    ri[:, 3] = rule["flags"]; ri[:, 7] = rule["admitted"]; ri[:, 11] = rule["drawn"]
    ri[:, 12] = np.where(real, rule["instance"], -1).astype(np.int64) & 0xFFFFFFFF
    ri[:, 13] = np.where(real, rule["primitive"], 0xFFFFFFFF)
    return rec


FIELDS = P.FIELDS


def compare(rule, got, counters=False):
    """Per record: ratio |record - rule| / bound of direct, unshadowed, emitted (the largest over the components; a NaN counts as inf; 0 on undecided records), and
    whether flags, lightsAdmitted, drawn, instance and primitive are exactly the rule's.  An undecided record is held to VALID, instance and primitive and to
    finite floats.  Records that are not real hits must equal the miss / bad-hit record word for word.  counters: the device ran with count_traversal, so the
    last two words are free; otherwise they are 0 everywhere."""
    got = np.asarray(got, dtype=np.float32); gi = got.view(np.uint32)
    want = as_records(rule); wi = want.view(np.uint32)
    real = rule["kind"] == 2
    decided = real & ~rule["undecided"]
    exact = (gi[:, 12] == wi[:, 12]) & (gi[:, 13] == wi[:, 13])
    exact &= np.where(decided, (gi[:, 3] == wi[:, 3]) & (gi[:, 7] == wi[:, 7]) & (gi[:, 11] == wi[:, 11]), (gi[:, 3] & (VALID | BAD_HIT)) == (wi[:, 3] & (VALID | BAD_HIT)))
    exact &= real | (gi == wi).all(axis=1)
    exact &= np.isfinite(got[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).all(axis=1)
    if not counters:
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


def outside(rule, got):
    """[N] bool: records that leave the rule's bound or differ in an integer."""
    ratios, exact = compare(rule, got)
    out = ~exact
    for r in ratios.values():
        out |= ~(r <= 1.0)
    return out


def shares(rule):
    """Of the real hits: (in shadow, more than one light drawn, noise factor 0, undecided)."""
    real = rule["kind"] == 2
    if not real.any():
        return (0.0,) * 4
    return (float(rule["in_shadow"][real].mean()), float((rule["draws"][real] > 1).mean()), float((rule["factor"][real] == 0).mean()), float(rule["undecided"][real].mean()))


def report(name, rule, ratios, exact):
    """One line per case, laid out like profiles/lighting_rule_deviation.txt."""
    real = rule["kind"] == 2
    n = int(real.sum())
    parts = ["%-24s hits %5d of %5d" % (name, n, len(real))]
    for k, _ in FIELDS:
        r = ratios[k][real]
        parts.append("%s max %.3f mean %.4f" % (k, r.max() if n else 0.0, r.mean() if n else 0.0))
    bound = max(float(rule[k][1][real].max()) if n else 0.0 for k, _ in FIELDS)
    sh = shares(rule)
    parts.append("largest bound %.2e  undecided %.4f %s  shadow %.3f multi %.3f factor-0 %.3f  redrawn %d  inexact %d" %
                 (bound, sh[3], rule["why"], sh[0], sh[1], sh[2], int(((rule["drawn"] >> 16) != 0).sum()), int((~exact).sum())))
    return "  ".join(parts)
