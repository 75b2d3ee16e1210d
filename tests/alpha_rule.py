"""Ray queries that honour alpha as a rule in numpy float64 (rules K1-K10).  TEST INFRASTRUCTURE.

`alpha_query_kernel` and `visibility_query_kernel` (csrc/alpha_query.hip) run an any-hit program inside the walk.  This module states what they must answer
without a walk of its own making decisions: the oracle's traversal (oracle/oracle_trace.c through tests/ray_rule.py's bindings) only *enumerates* -- brute
force over every triangle of every instance, with a callback that accepts nothing and never lowers tmax, so every intersection in tMin < t < tMax comes out
(geometry is bit-exact between oracle and device, so this is the candidate set a correct walk sees).  Everything about alpha comes from tests/material_rule.py:
each (ray, candidate) pair becomes a pseudo-hit and one call of `material_rule.materials` gives H6's alpha and flag at the ray's lod, H10's shadow alpha and
flag at level 0, each an `F` (value + float32 bound), and which candidates are undecided.  Rule O2 (K6) is restated here from the scene data.  The module imports
nothing from the library.

  closest_hit   K2: the closest decided candidate that is not a cutout; a ray with an undecided candidate at or before it is undecided.
  visibility    K5: max(1 - sum of a, 0) over the candidates that subtract, with bound sum(bounds) + (n + 1) U; 0 at an O2-opaque candidate.
"""
import ctypes as C

import numpy as np

import material_rule as M
import ray_rule
import surface_rule as S
from light_rule import U

CULL_BACK_FACING, ACCEPT_FIRST_HIT = ray_rule.CULL_BACK_FACING, ray_rule.ACCEPT_FIRST_HIT
VISIBILITY_VALID, VISIBILITY_BLOCKED = 0x1, 0x2
O2_THRESHOLD = 0.999

MUTATIONS = ("cutout_commits", "edge_on_every_shader", "cutout_at_level_0", "shadow_at_given_lod", "shadow_uses_solid_alpha", "o2_ignored",
             "stops_at_first_subtraction", "closest_only", "shadow_cutout_subtracts", "shadows_cull_back_faces")
CLOSEST_MUTATIONS = ("cutout_commits", "edge_on_every_shader", "cutout_at_level_0")


# ---- candidates ------------------------------------------------------------------------------------------------------------------------------

def candidates(oracle_scene, rays, cull=False, brute_force=True):
    """Every intersection of every Q6-valid ray within its window -> (ray index [M] int64, pseudo-hits (M, 8) float32 in RT64_RAY_HIT's layout), ordered by ray
    and, within a ray, by t (ties: instance, primitive)."""
    otrace = ray_rule._bind(oracle_scene.L)
    found = []

    def on_hit(user, hit, tmax, terminate):
        h = hit.contents
        found.append((h.t, h.u, h.v, h.instance, h.prim))
        return 0          # accepts nothing, lowers nothing
    cb = ray_rule.OAnyHitFn(on_hit)
    ray = ray_rule.ORay()
    ray.cullBackFaces = 1 if cull else 0
    index, rows = [], []
    for k, r in enumerate(np.asarray(rays, dtype=np.float32)):
        if not ray_rule.ray_is_valid(r):
            continue
        del found[:]
        ray.o[:] = [float(x) for x in r[0:3]]; ray.d[:] = [float(x) for x in r[4:7]]
        ray.tmin, ray.tmax = float(r[3]), float(r[7])
        otrace(oracle_scene.scene, C.byref(ray), 1 if brute_force else 0, cb, None, None)
        for h in sorted(found, key=lambda h: (h[0], h[3], h[4])):
            index.append(k); rows.append(h)
    hits = np.zeros((len(rows), 8), dtype=np.float32); hi = hits.view(np.uint32)
    if rows:
        a = np.array([(h[0], h[1], h[2]) for h in rows], dtype=np.float32)
        hits[:, 0:3] = a
        hi[:, 3] = np.array([h[3] for h in rows], dtype=np.uint32); hi[:, 4] = np.array([h[4] for h in rows], dtype=np.uint32)
    return np.array(index, dtype=np.int64), hits


# ---- K6: rule O2 from the scene data -----------------------------------------------------------------------------------------------------------

def shadow_opaque(data, levels, ignore=False):
    """[k] bool per ray-traced instance (hit `instance` k): does a shadow ray stop dead at it?  A shader without the alpha option: yes.  Otherwise a noise or
    texture-edge shader: no; an alpha formula that is neither a single input nor a product of two: no; else the smallest value the formula can take over the
    mesh's vertex alphas and the diffuse texture's texel alphas (every level), times shadowAlphaMultiplier, is compared with 0.999."""
    out = []
    for index in S.raytraced_instances(data):
        I = data.instances[index]
        shader_id = M.shader_of(data, I)[0]
        cc = M._combiner(shader_id)
        if ignore:
            out.append(False); continue
        if not cc["alpha"]:
            out.append(True); continue
        if cc["noise"] or cc["edge"] or not (cc["single1"] or cc["multiply1"]):
            out.append(False); continue
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
                a = np.concatenate([lv[..., 3].ravel() for lv in levels[I.diffuse]]).astype(np.float64) / 255.0
                return float(a.min()), float(a.max())
            return 1.0, 1.0
        c = cc["c"][1]
        if cc["single1"]:
            lo = bounds(c[3])[0]
        else:
            (l0, h0), (l2, h2) = bounds(c[0]), bounds(c[2])
            lo = min(l0 * l2, l0 * h2, h0 * l2, h0 * h2)
        product = float(I.material.shadowAlphaMultiplier) * lo
        # a case keeps its O2 products at least 0.01 away from the threshold, so that float32 and float64 agree on the side; the one exception is a product of
        # exactly 1 (vertex alpha 1, texel alpha 1, multiplier 1 -- the sample scene's), which is exact in both formats
        assert abs(product - O2_THRESHOLD) >= 0.01 or product == 1.0, (I.name, product)
        out.append(lo >= 0.0 and product >= O2_THRESHOLD)
    return np.array(out, dtype=bool)


def _edge(data):
    return np.array([M._combiner(M.shader_of(data, data.instances[i])[0])["edge"] for i in S.raytraced_instances(data)], dtype=bool)


def _spans(index, n):
    """first[k], last[k]: the rows of ray k in the ordered candidate list."""
    first = np.searchsorted(index, np.arange(n), side="left"); last = np.searchsorted(index, np.arange(n), side="right")
    return first, last


# ---- K2 ------------------------------------------------------------------------------------------------------------------------------------------

def closest_hit(data, levels, rays, cand, lods=None, mutate=None):
    """-> dict: hit (N, 8) float32 (t, u, v, instance, primitive; the miss record where nothing is accepted), ties {ray: rows of equal right} (K4), undecided [N],
    accepted [N] list of (M_k, 5) uint32 rows a walk that stops at the first accepted intersection may report, first_undecided [N], cutout_first [N] (the closest
    candidate is a decided cutout), candidates [N] (count)."""
    assert mutate is None or mutate in CLOSEST_MUTATIONS, mutate
    rays = np.asarray(rays, dtype=np.float32)
    n = len(rays)
    index, hits = cand
    lods = np.zeros(n, dtype=np.float32) if (lods is None or mutate == "cutout_at_level_0") else np.asarray(lods, dtype=np.float32)
    rule = M.materials(data, levels, rays[index], hits, lods[index])
    inst = hits.view(np.int32)[:, 3]
    edge = _edge(data)[inst] if len(inst) else np.zeros(0, dtype=bool)
    if mutate == "edge_on_every_shader":
        cut = np.where(edge, (rule["flags"] & M.CUTOUT) != 0, rule["color"][0][:, 3] <= M.EDGE); und = rule["undecided"].copy()
    else:
        cut = edge & ((rule["flags"] & M.CUTOUT) != 0); und = edge & rule["undecided"]          # every other shader commits whatever its alpha is
    bits = hits.view(np.uint32)
    out = np.zeros((n, 8), dtype=np.float32); ob = out.view(np.uint32)
    out[:, 0] = np.inf; ob[:, 3] = 0xFFFFFFFF; ob[:, 4] = 0xFFFFFFFF
    res = {"hit": out, "ties": {}, "undecided": np.zeros(n, dtype=bool), "accepted": [None] * n, "first_undecided": np.zeros(n, dtype=bool),
           "cutout_first": np.zeros(n, dtype=bool), "candidates": np.zeros(n, dtype=np.int64)}
    first, last = _spans(index, n)
    for k in range(n):
        a, b = first[k], last[k]
        res["candidates"][k] = b - a
        if a == b:
            res["accepted"][k] = np.zeros((0, 5), dtype=np.uint32); continue
        c, u = cut[a:b], und[a:b]
        res["cutout_first"][k] = bool(c[0] and not u[0])
        res["first_undecided"][k] = bool(u.any())
        res["accepted"][k] = bits[a:b, :5][~c | u]
        if mutate == "cutout_commits":
            ok = np.ones(b - a, dtype=bool)
        else:
            ok = ~c & ~u
        w = np.nonzero(ok)[0]
        if not len(w):
            res["undecided"][k] = bool(u.any()); continue
        j = w[0]
        t = hits[a + j, 0]
        res["undecided"][k] = bool(u[hits[a:b, 0] <= t].any())
        ob[k, :5] = bits[a + j, :5]
        same = w[hits[a + w, 0] == t]
        if len(same) > 1:
            res["ties"][k] = bits[a + same, :5]
    return res


def closest_matches(rule, got):
    """[N] bool: t, u, v bit-equal and instance, primitive exact on every decided ray (any of the tied rows, K4); an undecided ray matches."""
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)[:, :5]
    ok = (g == rule["hit"].view(np.uint32)[:, :5]).all(axis=1)
    for k, rows in rule["ties"].items():
        ok[k] = bool((rows == g[k]).all(axis=1).any())
    return ok | rule["undecided"]


def first_matches(rule, got):
    """[N] bool under ACCEPT_FIRST_HIT: the hit is a member of the accepted set, a miss exactly where the set is empty; rays with an undecided candidate are held to
    membership only."""
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)
    ok = np.zeros(len(g), dtype=bool)
    for k in range(len(g)):
        acc = rule["accepted"][k]
        missed = g[k, 3] == 0xFFFFFFFF
        if missed:
            ok[k] = len(acc) == 0 or bool(rule["first_undecided"][k])
        else:
            ok[k] = bool(len(acc) and (acc == g[k, :5]).all(axis=1).any())
    return ok


# ---- K5 ------------------------------------------------------------------------------------------------------------------------------------------

def visibility(data, levels, rays, cand, mutate=None, lods=None):
    """-> dict: v, e [N] (value and bound of the visibility), undecided [N], by_o2 [N] (0 because of a decided O2-opaque candidate), subtracting [N] (count of
    candidates that subtract), valid [N] (Q6)."""
    assert mutate is None or (mutate in MUTATIONS and mutate not in CLOSEST_MUTATIONS), mutate
    rays = np.asarray(rays, dtype=np.float32)
    n = len(rays)
    index, hits = cand
    if mutate == "shadow_at_given_lod":
        rule = M.materials(data, levels, rays[index], hits, np.asarray(lods, dtype=np.float32)[index], mutate="shadow_at_given_lod")
    else:
        rule = M.materials(data, levels, rays[index], hits)          # H10: level 0 whatever the ray's lod
    inst = hits.view(np.int32)[:, 3]
    opaque = shadow_opaque(data, levels, ignore=(mutate == "o2_ignored"))
    opaque = opaque[inst] if len(inst) else np.zeros(0, dtype=bool)
    if mutate == "shadow_uses_solid_alpha":
        a, ae, cut = rule["color"][0][:, 3], rule["color"][1][:, 3], (rule["flags"] & M.CUTOUT) != 0
    else:
        a, ae, cut = rule["shadow"][0][:, 0], rule["shadow"][1][:, 0], (rule["flags"] & M.SHADOW_CUTOUT) != 0
    if mutate == "shadow_cutout_subtracts":
        cut = np.zeros_like(cut)
    und = rule["undecided"] & ~opaque
    res = {"v": np.ones(n), "e": np.zeros(n), "undecided": np.zeros(n, dtype=bool), "by_o2": np.zeros(n, dtype=bool), "subtracting": np.zeros(n, dtype=np.int64),
           "valid": np.array([ray_rule.ray_is_valid(r) for r in rays], dtype=bool)}
    first, last = _spans(index, n)
    for k in range(n):
        s0, s1 = first[k], last[k]
        if s0 == s1:
            continue
        if mutate in ("closest_only", "stops_at_first_subtraction"):
            rows = np.arange(s0, s1)
            if mutate == "stops_at_first_subtraction":
                rows = rows[opaque[rows] | ~cut[rows]]
            s0, s1 = (rows[0], rows[0] + 1) if len(rows) else (s0, s0)
            if s0 == s1:
                continue
        if opaque[s0:s1].any():
            res["v"][k] = 0.0; res["by_o2"][k] = True; continue
        if und[s0:s1].any():
            res["undecided"][k] = True; continue
        sub = ~cut[s0:s1]
        m = int(sub.sum())
        res["subtracting"][k] = m
        s = 1.0 - float(a[s0:s1][sub].sum())
        e = float(ae[s0:s1][sub].sum()) + (m + 1) * U
        v = min(max(s, 0.0), 1.0)
        res["v"][k] = v
        res["e"][k] = max(min(max(s + e, 0.0), 1.0) - v, v - min(max(s - e, 0.0), 1.0))
    return res


def visibility_check(rule, got):
    """-> (ratio [N]: |got - v| / e on decided rays (0 where equal, inf outside a zero bound), ok [N]: flags and ranges as K1 / K5 state them)."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    vis, flags = got[:, 0].astype(np.float64), got.view(np.uint32)[:, 1]
    diff = np.abs(vis - rule["v"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / rule["e"])
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    ratio = np.where(rule["undecided"], 0.0, ratio)
    ok = np.isfinite(vis) & (vis >= 0.0) & (vis <= 1.0)
    ok &= np.where(rule["valid"], (flags & VISIBILITY_VALID) != 0, (flags == 0) & (vis == 1.0))
    ok &= ((flags & VISIBILITY_BLOCKED) != 0) == (vis == 0.0)                       # the flag says what the number says ...
    sure_open = ~rule["undecided"] & (rule["v"] - rule["e"] > 0.0)
    sure_shut = ~rule["undecided"] & (rule["v"] == 0.0) & (rule["e"] == 0.0)       # (0 by O2, or a sum that no rounding brings under 1)
    ok &= ~sure_open | ((flags & VISIBILITY_BLOCKED) == 0)                          # ... and is the rule's wherever the rule's interval excludes 0 or is 0 exactly
    ok &= ~sure_shut | ((flags & VISIBILITY_BLOCKED) != 0)
    return ratio, ok
