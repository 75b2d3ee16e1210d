"""A ray's sorted hit list and each layer's weight as a rule in numpy float64 (rules T1-T12).  TEST INFRASTRUCTURE.

`layer_walk_kernel` and `layer_weight_kernel` (csrc/layers.hip) build and resolve the list a frame keeps per ray.  This module states what they must answer from
candidates that are only enumerated: `alpha_rule.candidates` (brute force over every triangle, a callback that accepts nothing) gives every intersection of a ray's
window, `material_rule.materials` the alpha of each with its float32 bound, and rule O1 is restated here from the scene data as `alpha_rule.shadow_opaque` restates
O2.  The module imports nothing from the library.

  T2 / T4 are single float32 operations on bit-exact inputs (t, depthBias, maxDepthBias), so keys and reach limits are restated in float32 and carry no bound; a ray
  is undecided where two keys that matter are bit-equal (T2 allows either order) or an intersection lies within two ulps of a reach limit.
  T5's classes, as this rule decides them: (a) fewer than 16 accepted intersections in the ray's window -- nothing is ever displaced, so the list is the accepted
  intersections with key < key_E, sorted, then E, whatever the order of arrival; (b) 16 or more, all on instances of one depthBias -- key order is t order, so what
  slot 15 commits and what an opaque hit cuts off lies behind the 16 smallest keys; (c) otherwise -- the oracle's ordered walk (`ordered_walk`: ray_rule's otrace with
  brute_force = 0 and a Python callback that restates rt64_shader.cpp:547-581 and lowers tmax through its pointer).
  T7 in float64: a is the UNORM8 step of the alpha (undecided within its bound of a rounding boundary, or of 0.3 on an edge shader); weights carry the bound
  (n + 1) 2^-24 relative per step, n the operations behind them.
"""
import ctypes as C

import numpy as np

import material_rule as M
import ray_rule
import surface_rule as S
from light_rule import U

LAYERS_MAX = 16
LAYERS_VALID, LAYERS_ENDS_OPAQUE, LAYERS_FULL = 0x1, 0x2, 0x4
COVERAGE_VALID, COVERAGE_COVERED, COVERAGE_GLASS, COVERAGE_BAD_HIT = 0x1, 0x2, 0x4, 0x8
O1_THRESHOLD = np.float32(0.999)
EPSILON = float(np.float32(1e-6))
F32 = np.float32

MUTATIONS = ("sorted_by_t", "no_truncation", "cutouts_kept", "opaque_ignores_multiplier", "weights_unquantised", "glass_does_not_end", "skipped_layer_scales_rem",
             "covered_never_stops")


# ---- T3: rule O1 from the scene data -------------------------------------------------------------------------------------------------------------

def o1_opaque(data, levels, mutate=None):
    """[k] bool per ray-traced instance: did the frame prove it opaque?  A noise or texture-edge shader: no.  Without the alpha option the bound is 1; otherwise the
    alpha formula must be a single input or a product of two, and the bound is its smallest value over the mesh's vertex alphas and the diffuse texels.  Opaque when
    bound x solidAlphaMultiplier >= 0.999 in float32."""
    out = []
    for index in S.raytraced_instances(data):
        I = data.instances[index]
        shader_id = M.shader_of(data, I)[0]
        cc = M._combiner(shader_id)
        if cc["noise"] or cc["edge"]:
            out.append(False); continue
        if not cc["alpha"]:
            lo = 1.0
        elif not (cc["single1"] or cc["multiply1"]):
            out.append(False); continue
        else:
            mesh = data.meshes[I.mesh]
            layout = S.vertex_layout(shader_id)
            first = layout["uv"] + (8 if layout["has_uv"] else 0)
            every = np.arange(len(mesh.vertices))

            def bounds(item):
                if item == 0:
                    return 0.0, 0.0
                if item <= 4:
                    a = S._fetch(mesh, layout, every, first + (item - 1) * 16 + 12, 1)
                    return float(a.min()), float(a.max())
                if item <= 6:
                    a = np.concatenate([lv[..., 3].ravel() for lv in levels[I.diffuse][:1]]).astype(np.float32) / F32(255.0)
                    return float(a.min()), float(a.max())
                return 1.0, 1.0
            c = cc["c"][1]
            if cc["single1"]:
                lo = bounds(c[3])[0]
            else:
                (l0, h0), (l2, h2) = bounds(c[0]), bounds(c[2])
                lo = min(F32(l0) * F32(l2), F32(l0) * F32(h2), F32(h0) * F32(l2), F32(h0) * F32(h2))
        mult = F32(1.0) if mutate == "opaque_ignores_multiplier" else F32(I.material.solidAlphaMultiplier)
        out.append(bool(lo >= 0.0 and mult * F32(lo) >= O1_THRESHOLD))
    return np.array(out, dtype=bool)


def instance_table(data, levels, mutate=None):
    """Per ray-traced instance: depthBias (float32), O1, refractionFactor, edge; and the frame's maxDepthBias (float32)."""
    rt = S.raytraced_instances(data)
    bias = np.array([F32(data.instances[i].material.depthBias) for i in rt], dtype=np.float32)
    refr = np.array([float(data.instances[i].material.refractionFactor) for i in rt])
    edge = np.array([M._combiner(M.shader_of(data, data.instances[i])[0])["edge"] for i in rt], dtype=bool)
    return {"bias": bias, "opaque": o1_opaque(data, levels, mutate), "refraction": refr, "edge": edge, "max_bias": F32(bias.max()) if len(bias) else F32(0.0)}


# ---- T1-T6 ---------------------------------------------------------------------------------------------------------------------------------------

def _insert(keys, rows, key, row):
    """trace_surface<true>'s insertion into 16 slots (+ the scratch slot, dropped): -> the slot the entry landed in, or 16."""
    hi = min(len(keys), LAYERS_MAX)
    while hi > 0 and key < keys[hi - 1]:
        hi -= 1
    if hi < LAYERS_MAX:
        keys.insert(hi, key); rows.insert(hi, row)
        del keys[LAYERS_MAX:]; del rows[LAYERS_MAX:]
    return hi


def ordered_walk(oracle_scene, ray, cull, accepted_of, table):
    """T5 (c): the oracle's ordered walk of one ray with the frame's any-hit restated.  accepted_of: (instance, primitive) -> candidate row, for the accepted
    intersections of the ray.  -> candidate rows in list order, 16 at most (not yet truncated)."""
    otrace = ray_rule._bind(oracle_scene.L)
    keys, rows = [], []

    def on_hit(user, hit, tmax, terminate):
        h = hit.contents
        row = accepted_of.get((int(h.instance), int(h.prim)))
        if row is None:
            return 0                                          # IgnoreHit() before the hit is stored
        t = F32(h.t)
        key = F32(t - table["bias"][h.instance])
        hi = _insert(keys, rows, key, row)
        if hi < LAYERS_MAX and hi == LAYERS_MAX - 1 and t < F32(tmax[0]):
            tmax[0] = float(t)
        if table["opaque"][h.instance]:
            lim = F32(key + table["max_bias"])
            if lim < F32(tmax[0]):
                tmax[0] = float(lim)
        return 0
    cb = ray_rule.OAnyHitFn(on_hit)
    r = ray_rule.ORay()
    r.cullBackFaces = 1 if cull else 0
    r.o[:] = [float(x) for x in ray[0:3]]; r.d[:] = [float(x) for x in ray[4:7]]
    r.tmin, r.tmax = float(ray[3]), float(ray[7])
    otrace(oracle_scene.scene, C.byref(r), 0, cb, None, None)
    return rows


def lists(data, levels, rays, cand, lods=None, cull=False, oracle_scene=None, mutate=None):
    """-> dict: rows [N] (candidate rows in list order, truncated by T3, 16 at most), cls [N] ('a', 'b', 'c' or '' for an invalid ray), undecided [N], ends_opaque
    [N], full [N], valid [N], alpha (value, bound per candidate), quantum (the UNORM8 step per candidate, -1 where undecided), table.  Class (c) rays need
    `oracle_scene`; without it they are marked undecided."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rays = np.asarray(rays, dtype=np.float32)
    n = len(rays)
    index, hits = cand
    lods = np.zeros(n, dtype=np.float32) if lods is None else np.asarray(lods, dtype=np.float32)
    table = instance_table(data, levels, mutate)
    mat = M.materials(data, levels, rays[index], hits, lods[index])
    inst = hits.view(np.int32)[:, 3].astype(np.int64)
    prim = hits.view(np.uint32)[:, 4].astype(np.int64)
    edge = table["edge"][inst] if len(inst) else np.zeros(0, dtype=bool)
    cut = edge & ((mat["flags"] & M.CUTOUT) != 0)
    und_accept = edge & mat["undecided"]
    if mutate == "cutouts_kept":
        cut = np.zeros_like(cut)
    t = hits[:, 0]
    bias = table["bias"][inst] if len(inst) else np.zeros(0, dtype=np.float32)
    key = (t - bias).astype(np.float32) if mutate != "sorted_by_t" else t.copy()
    opaque = table["opaque"][inst] if len(inst) else np.zeros(0, dtype=bool)
    alpha_v, alpha_e = mat["color"][0][:, 3].copy(), mat["color"][1][:, 3].copy()
    # the frame's UNORM8 store of the alpha: floor(a 255 + 0.5) in float32
    scaled = alpha_v * 255.0 + 0.5
    quantum = np.floor(scaled)
    frac_margin = np.minimum(scaled - quantum, quantum + 1.0 - scaled)
    und_alpha = mat["undecided"] | ((frac_margin < 255.0 * M.DECISION_K * alpha_e + 4 * 256 * U) & (alpha_v > 0.0) & (alpha_v < 1.0))
    quantum = np.clip(quantum, 0, 255)
    res = {"rows": [None] * n, "cls": [""] * n, "undecided": np.zeros(n, dtype=bool), "ends_opaque": np.zeros(n, dtype=bool), "full": np.zeros(n, dtype=bool),
           "valid": np.array([ray_rule.ray_is_valid(r) for r in rays], dtype=bool), "alpha": (alpha_v, alpha_e), "quantum": quantum, "und_alpha": und_alpha,
           "table": table, "cand": cand, "opaque": opaque, "key": key}
    first = np.searchsorted(index, np.arange(n), side="left"); last = np.searchsorted(index, np.arange(n), side="right")
    for k in range(n):
        a, b = first[k], last[k]
        res["rows"][k] = np.zeros(0, dtype=np.int64)
        if not res["valid"][k]:
            continue
        acc = np.arange(a, b)[~cut[a:b]]
        res["undecided"][k] = bool(und_accept[a:b].any())
        res["cls"][k] = "a"
        if not len(acc):
            continue
        one_bias = bool((bias[acc] == bias[acc[0]]).all())
        cls = "a" if len(acc) < LAYERS_MAX else ("b" if one_bias else "c")
        res["cls"][k] = cls
        if cls == "c":
            if oracle_scene is None:
                res["undecided"][k] = True; continue
            order = np.array(ordered_walk(oracle_scene, rays[k], cull, {(int(inst[r]), int(prim[r])): int(r) for r in acc}, table), dtype=np.int64)
        else:
            order = acc[np.argsort(key[acc], kind="stable")]
            ks = key[order]
            first_opaque = np.nonzero(opaque[order])[0]
            upto = first_opaque[0] + 1 if len(first_opaque) else len(order)
            upto = min(upto + 1, len(order), LAYERS_MAX + 1)
            if (ks[1:upto] == ks[:upto - 1]).any():
                res["undecided"][k] = True                    # T2: bit-equal keys may come out either way
            # an intersection within two ulps of an opaque hit's reach may or may not have been seen; it matters only in front of the list's end
            for e in order[opaque[order]][:1]:
                lim = F32(key[e] + table["max_bias"])
                near = (np.abs(t[acc].astype(np.float64) - float(lim)) <= 2.0 * float(np.spacing(lim))) & (acc != e)
                if near.any() and (key[acc][near] <= key[e]).any():
                    res["undecided"][k] = True
            order = order[:LAYERS_MAX]
        if mutate != "no_truncation":
            op = np.nonzero(opaque[order])[0]
            if len(op):
                order = order[:op[0] + 1]; res["ends_opaque"][k] = True
        elif len(order) and opaque[order[-1]]:
            res["ends_opaque"][k] = True
        res["full"][k] = len(order) == LAYERS_MAX and not res["ends_opaque"][k]
        res["rows"][k] = order
    return res


def hit_records(rule, max_layers=LAYERS_MAX):
    """The lists as RT64_TraceViewRayLayers writes them: hits (L, N, 8) float32 (the miss record behind a list's end, counters 0) and layers (N, 2) uint32 (count, flags)."""
    index, hits = rule["cand"]
    n = len(rule["rows"])
    out = np.zeros((max_layers, n, 8), dtype=np.float32); ob = out.view(np.uint32)
    out[:, :, 0] = np.inf; ob[:, :, 3] = 0xFFFFFFFF; ob[:, :, 4] = 0xFFFFFFFF
    lay = np.zeros((n, 2), dtype=np.uint32)
    hb = hits.view(np.uint32)
    for k, rows in enumerate(rule["rows"]):
        m = min(len(rows), max_layers)
        for l in range(m):
            ob[l, k, :5] = hb[rows[l], :5]
        lay[k, 0] = m
        if rule["valid"][k]:
            lay[k, 1] = LAYERS_VALID | (LAYERS_ENDS_OPAQUE if rule["ends_opaque"][k] else 0) | (LAYERS_FULL if rule["full"][k] else 0)
    return out, lay


# ---- T7 ------------------------------------------------------------------------------------------------------------------------------------------

def weights(rule, max_layers=LAYERS_MAX, mutate=None, bad_tail=None):
    """T7 over the rule's own lists (bad_tail [N] bool: a record with an out-of-range index follows the list, where it is shorter than max_layers) -> dict: w, e (L, N) value and bound of every weight, transmittance / refraction (value, bound) [N], shaded [N], flags [N],
    undecided [N] (an alpha on a rounding boundary, or a decision within its bound)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    n = len(rule["rows"])
    index, hits = rule["cand"]
    inst = hits.view(np.int32)[:, 3].astype(np.int64)
    table = rule["table"]
    alpha_v = rule["alpha"][0]
    w = np.zeros((max_layers, n)); e = np.zeros((max_layers, n))
    out = {"w": w, "e": e, "transmittance": (np.ones(n), np.zeros(n)), "refraction": (np.zeros(n), np.zeros(n)), "shaded": np.zeros(n, dtype=np.int64),
           "flags": np.zeros(n, dtype=np.int64), "undecided": rule["undecided"].copy()}
    for k, rows in enumerate(rule["rows"]):
        if not rule["valid"][k]:
            continue
        flags, rem, ops, refr, refr_ops, shaded = COVERAGE_VALID, 1.0, 0, 0.0, 0, 0
        for l, r in enumerate(rows[:max_layers]):
            if rule["und_alpha"][r]:
                out["undecided"][k] = True
            a = float(alpha_v[r]) if mutate == "weights_unquantised" else float(F32(rule["quantum"][r]) / F32(255.0))
            wl = rem * a
            bound = (ops + 2) * U * wl
            if abs(wl - EPSILON) <= bound + 2 * U * EPSILON:
                out["undecided"][k] = True
            if wl >= EPSILON:
                w[l, k], e[l, k] = wl, bound
                rem *= (1.0 - a); ops += 2; shaded += 1
                if table["refraction"][inst[r]] > EPSILON and mutate != "glass_does_not_end":
                    refr, refr_ops, rem = rem, ops, 0.0; flags |= COVERAGE_GLASS
            elif mutate == "skipped_layer_scales_rem":
                rem *= (1.0 - a); ops += 2
            if rem != 0.0 and abs(rem - EPSILON) <= (ops + 1) * U * rem + 2 * U * EPSILON:
                out["undecided"][k] = True
            if rem <= EPSILON:
                flags |= COVERAGE_COVERED
                if mutate != "covered_never_stops":
                    break
        else:
            if bad_tail is not None and bad_tail[k] and len(rows) < max_layers:
                flags |= COVERAGE_BAD_HIT                     # the resolve was still open when it reached the record
        out["transmittance"][0][k], out["transmittance"][1][k] = rem, (ops + 1) * U * rem
        out["refraction"][0][k], out["refraction"][1][k] = refr, (refr_ops + 1) * U * refr
        out["shaded"][k], out["flags"][k] = shaded, flags
    return out


def compare(rule, wrule, got_hits, got_layers, got_weights=None, got_coverage=None, max_layers=LAYERS_MAX):
    """-> dict of [N] bool / float arrays on decided rays: lists (indices, t, u, v bits, count and flags exact), ratio (largest |weight - rule| / bound of a ray, its
    transmittance and refraction included), coverage (shaded and flags exact).  Undecided rays pass."""
    want_hits, want_lay = hit_records(rule, max_layers)
    gh = np.ascontiguousarray(got_hits, dtype=np.float32).view(np.uint32)
    gl = np.ascontiguousarray(got_layers).view(np.uint32)
    und = rule["undecided"]
    res = {"lists": ((gh[:, :, :5] == want_hits.view(np.uint32)[:, :, :5]).all(axis=(0, 2)) & (gl[:, 0] == want_lay[:, 0]) & (gl[:, 1] == want_lay[:, 1])) | und}
    if got_weights is None:
        return res
    und_w = wrule["undecided"]
    gw = np.asarray(got_weights, dtype=np.float64); gc = np.ascontiguousarray(got_coverage, dtype=np.float32)

    def ratio(got, v, e):
        d = np.abs(got - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d == 0.0, 0.0, d / e)
        return np.where(np.isnan(r), np.inf, r)
    r = ratio(gw, wrule["w"], wrule["e"]).max(axis=0)
    r = np.maximum(r, ratio(gc[:, 0].astype(np.float64), *wrule["transmittance"]))
    r = np.maximum(r, ratio(gc[:, 1].astype(np.float64), *wrule["refraction"]))
    res["ratio"] = np.where(und_w, 0.0, r)
    cb = gc.view(np.uint32)
    res["coverage"] = ((cb[:, 2] == wrule["shaded"]) & (cb[:, 3] == wrule["flags"])) | und_w
    return res
