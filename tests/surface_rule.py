"""Surface records of ray-query hits as a rule in numpy float64 (rules A1-A8).  TEST INFRASTRUCTURE.

`hit_surface_kernel` (csrc/surface.hip) makes its records with the device functions the frame's any-hit program runs (inst_view,
get_vertex_data of csrc/shade.h).  This module states the same operation from its meaning: the hit's triangle in the mesh as the host
sent it, barycentric interpolation, the instance's transform for points and its inverse transpose for normals, the flip towards the ray.
It reads a `SceneData`, the rays and the hits; it imports nothing from oracle/ and nothing from the library.

Every value is an `F` of tests/light_rule.py: a float64 value and a first-order bound on what a float32 evaluation of the same expression
(correctly rounded +, -, *; 1-ulp rsqrt) may differ by.  A6's sign is a decision: where |dot(geometricNormal, direction)| is below
DECISION_K x its own error the hit is *undecided*, and a record is compared up to the joint flip of its BACK_FACE flag and shading normal.
"""
import numpy as np

import light_rule as L
from light_rule import F

VALID, BACK_FACE, HAS_UV, BAD_HIT = 0x1, 0x2, 0x4, 0x8
DECISION_K = L.DECISION_K
# objectToWorldNormal = transpose(inverse(upper 3x3 of the transform)).  The host's mat_inverse expands cofactors in double and rounds each entry to float32 once: the
# rounding is U x |entry|; in front of it each entry is a quotient of a 6-term sum of triple products (12 multiplies, 5 additions), a 4-term determinant (4 + 3), one
# reciprocal and one product -- 26 double operations, taken as INVERSE_OPS = 32 roundings of 2^-53, each amplified at most by the inverse's own condition, entrywise
# |M^-1| |M| |M^-1| (the first-order perturbation of an inverse: d(M^-1) = -M^-1 dM M^-1).
INVERSE_OPS = 32
D = 2.0 ** -53

MUTATIONS = ("uv_swapped", "b0_on_p1", "normal_by_object_to_world", "no_flip", "flip_geometric", "no_zero_fallback", "no_renormalise")

MESH_RAYTRACE_ENABLED = 0x1


def raytraced_instances(data):
    """Hit `instance` k is the k-th instance, in creation order, whose mesh is ray traced."""
    return [i for i, inst in enumerate(data.instances) if data.meshes[inst.mesh].flags & MESH_RAYTRACE_ENABLED]


def vertex_layout(shader_id):
    """Byte layout of a vertex as the shader reads it: float4 position, float3 normal, float2 uv when either combiner cycle reads a texture (slots 5, 6: texture 0;
    7: texture 1), then one float3 (float4 with the alpha option, bit 24) per vertex input the combiner names (slots 1-4)."""
    slots = [(shader_id >> (3 * i)) & 7 for i in range(8)]
    has_uv = any(s in (5, 6, 7) for s in slots)
    inputs = max([s for s in slots if 1 <= s <= 4], default=0)
    size = 16 + 12 + (8 if has_uv else 0) + inputs * (16 if shader_id & (1 << 24) else 12)
    return {"normal": 16, "uv": 28, "has_uv": has_uv, "size": size}


def _fetch(mesh, layout, vertex, offset, n):
    """n floats at byte `offset` of vertices `vertex`, the array strided by the layout's vertex size (as the shader strides it)."""
    raw = np.frombuffer(np.ascontiguousarray(mesh.vertices).tobytes(), dtype=np.uint8)
    at = vertex.astype(np.int64)[:, None] * layout["size"] + offset + np.arange(4 * n)[None, :]
    return np.ascontiguousarray(raw[at]).view(np.float32).astype(np.float64)


def _vecF(x):
    return [F(x[:, 0]), F(x[:, 1]), F(x[:, 2])]


def _mul_vector(M, p):
    """p * M with w = 0, left to right; M: 3 x 3 list of F or floats (row-vector convention)."""
    return [L.add(L.add(L.mul(p[0], M[0][c]), L.mul(p[1], M[1][c])), L.mul(p[2], M[2][c])) for c in range(3)]


def _normal_matrix(transform):
    """transpose(inverse(upper 3 x 3)) as 3 x 3 F: value in float64, error = the float32 rounding of each entry + the double arithmetic in front of it."""
    m = np.asarray(transform, dtype=np.float64)[:3, :3]
    inv = np.linalg.inv(m)
    err = L.U * np.abs(inv) + INVERSE_OPS * D * (np.abs(inv) @ np.abs(m) @ np.abs(inv))
    n, e = inv.T, err.T
    return [[F(n[r, c], e[r, c]) for c in range(3)] for r in range(3)]


def _interp(a, b):
    """(a0 b0 + a1 b1) + a2 b2 per component; a: three (N, k) arrays of exact values, b: three F."""
    k = a[0].shape[1]
    return [L.add(L.add(L.mul(F(a[0][:, c]), b[0]), L.mul(F(a[1][:, c]), b[1])), L.mul(F(a[2][:, c]), b[2])) for c in range(k)]


def _stack(fs):
    return np.stack([f.v for f in fs], axis=1), np.stack([np.broadcast_to(f.e, f.v.shape) for f in fs], axis=1)


def surfaces(data, rays, hits, mutate=None):
    """-> dict of per-record arrays: kind (0 miss, 1 bad hit, 2 real), position / geometric / shading / uv as (value, bound) pairs of (N, k) float64, back (bool),
    undecided (bool), has_uv (bool), instance, primitive (int64), t (float32 bits as uint32)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rays = np.asarray(rays, dtype=np.float32); hits = np.asarray(hits, dtype=np.float32)
    n = len(rays)
    hi = hits.view(np.int32); hu = hits.view(np.uint32)
    inst = hi[:, 3].astype(np.int64); prim = hu[:, 4].astype(np.int64)
    rt = raytraced_instances(data)
    layout = vertex_layout(data.shader_id)
    out = {"kind": np.zeros(n, dtype=np.int64), "back": np.zeros(n, dtype=bool), "undecided": np.zeros(n, dtype=bool), "has_uv": np.zeros(n, dtype=bool),
           "instance": inst, "primitive": prim, "t": hu[:, 0].copy()}
    for name, k in (("position", 3), ("geometric", 3), ("shading", 3), ("uv", 2)):
        out[name] = (np.zeros((n, k)), np.zeros((n, k)))
    out["kind"][inst >= 0] = 1                                     # A3 until shown to be in range
    for k, index in enumerate(rt):
        I = data.instances[index]
        mesh = data.meshes[I.mesh]
        tri_count = len(mesh.indices) // 3
        sel = np.nonzero((inst == k) & (prim < tri_count))[0]
        if not len(sel):
            continue
        out["kind"][sel] = 2
        u, v = F(hits[sel, 1].astype(np.float64)), F(hits[sel, 2].astype(np.float64))
        if mutate == "uv_swapped":
            u, v = v, u
        b = [L.sub(L.sub(1.0, u), v), u, v]                        # A4
        if mutate == "b0_on_p1":
            b = [b[1], b[0], b[2]]
        corner = [np.asarray(mesh.indices, dtype=np.int64)[3 * prim[sel] + c] for c in range(3)]
        p = [_fetch(mesh, layout, corner[c], 0, 3) for c in range(3)]
        nr = [_fetch(mesh, layout, corner[c], layout["normal"], 3) for c in range(3)]
        T = np.asarray(I.transform, dtype=np.float32).astype(np.float64)
        obj = _interp(p, b)
        world = [L.add(L.add(L.add(L.mul(obj[0], T[0, c]), L.mul(obj[1], T[1, c])), L.mul(obj[2], T[2, c])), T[3, c]) for c in range(3)]
        out["position"][0][sel], out["position"][1][sel] = _stack(world)
        # A5: tn = -cross(p2 - p0, p1 - p0), through the inverse transpose, normalised
        tn = L.neg3(L.cross3(L.sub3(_vecF(p[2]), _vecF(p[0])), L.sub3(_vecF(p[1]), _vecF(p[0]))))
        N = [[float(T[r, c]) for c in range(3)] for r in range(3)] if mutate == "normal_by_object_to_world" else _normal_matrix(T)
        gn = L.normalize3(_mul_vector(N, tn))
        # A6
        d = rays[sel, 4:7].astype(np.float64)
        dot = L.dot3(gn, _vecF(d))
        back = dot.v > 0.0
        out["undecided"][sel] = np.abs(dot.v) < DECISION_K * dot.e
        out["back"][sel] = back
        # A7
        vn = _interp(nr, b)
        zero = (vn[0].v == 0.0) & (vn[1].v == 0.0) & (vn[2].v == 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            unit = L.normalize3(vn)
        if mutate != "no_zero_fallback":
            unit = [L.where(zero, tn[c], unit[c]) for c in range(3)]
        with np.errstate(divide="ignore", invalid="ignore"):
            moved = _mul_vector(N, unit)
            sn = moved if mutate == "no_renormalise" else L.normalize3(moved)
        sign = np.where(back, -1.0, 1.0)
        if mutate != "no_flip":
            sn = [F(c.v * sign, c.e) for c in sn]
        if mutate == "flip_geometric":
            gn = [F(c.v * sign, c.e) for c in gn]
        out["geometric"][0][sel], out["geometric"][1][sel] = _stack(gn)
        out["shading"][0][sel], out["shading"][1][sel] = _stack(sn)
        # A8
        if layout["has_uv"]:
            t = [_fetch(mesh, layout, corner[c], layout["uv"], 2) for c in range(3)]
            uv = [L.add(L.add(L.mul(F(t[0][:, c]), b[0]), L.mul(F(t[1][:, c]), b[1])), L.mul(F(t[2][:, c]), b[2])) for c in range(2)]
            out["uv"][0][sel], out["uv"][1][sel] = _stack(uv)
            out["has_uv"][sel] = True
    return out


def as_records(rule):
    """The rule's own values in RT64_RAY_SURFACE's layout, (N, 16) float32 (what a float32 evaluation with no error at all would store)."""
    n = len(rule["kind"])
    rec = np.zeros((n, 16), dtype=np.float32); ri = rec.view(np.uint32)
    real = rule["kind"] == 2
    rec[:, 0:3] = rule["position"][0]; rec[:, 4:7] = rule["geometric"][0]; rec[:, 8:11] = rule["shading"][0]; rec[:, 12:14] = rule["uv"][0]
    ri[:, 3] = np.where(real, VALID | np.where(rule["back"], BACK_FACE, 0) | np.where(rule["has_uv"], HAS_UV, 0), np.where(rule["kind"] == 1, BAD_HIT, 0))
    ri[:, 7] = np.where(real, rule["instance"], -1).astype(np.int64) & 0xFFFFFFFF
    ri[:, 11] = np.where(real, rule["primitive"], 0xFFFFFFFF)
    ri[:, 14] = np.where(real, rule["t"], np.float32(np.inf).view(np.uint32))
    return rec


def compare(rule, got):
    """Per record: ratio |record - rule| / bound of position, geometric normal, shading normal, uv (the largest over the components; a NaN counts as inf), and whether
    flags, instance, primitive, t and reserved are exactly the rule's.  An undecided hit is held to the orientation its own BACK_FACE flag names.  Records that are
    not real hits must equal the miss / bad-hit record word for word."""
    got = np.asarray(got, dtype=np.float32); gi = got.view(np.uint32)
    want = as_records(rule); wi = want.view(np.uint32)
    real = rule["kind"] == 2
    flip = real & rule["undecided"] & (((gi[:, 3] ^ wi[:, 3]) & BACK_FACE) != 0)
    wi[flip, 3] ^= BACK_FACE
    sv = rule["shading"][0].copy(); sv[flip] = -sv[flip]
    exact = (gi[:, 3] == wi[:, 3]) & (gi[:, 7] == wi[:, 7]) & (gi[:, 11] == wi[:, 11]) & (gi[:, 14] == wi[:, 14]) & (gi[:, 15] == 0)
    exact &= real | (gi == wi).all(axis=1)
    ratios = {}
    for name, cols, v, e in (("position", slice(0, 3), rule["position"][0], rule["position"][1]), ("geometric", slice(4, 7), rule["geometric"][0], rule["geometric"][1]),
                             ("shading", slice(8, 11), sv, rule["shading"][1]), ("uv", slice(12, 14), rule["uv"][0], rule["uv"][1])):
        diff = np.abs(got[:, cols].astype(np.float64) - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff == 0.0, 0.0, diff / e)
        r = np.where(np.isnan(r), np.inf, r).max(axis=1)
        ratios[name] = np.where(real, r, 0.0)
    return ratios, exact


def report(name, rule, ratios, exact):
    """One line per case, laid out like profiles/light_rule_deviation.txt."""
    real = rule["kind"] == 2
    n = int(real.sum())
    parts = ["%-28s hits %5d of %5d" % (name, n, len(real))]
    for k in ("position", "geometric", "shading", "uv"):
        r = ratios[k][real]
        parts.append("%s max %.3f mean %.4f" % (k, r.max() if n else 0.0, r.mean() if n else 0.0))
    parts.append("undecided %.4f" % (float(rule["undecided"][real].mean()) if n else 0.0))
    parts.append("inexact %d" % int((~exact).sum()))
    return "  ".join(parts)
