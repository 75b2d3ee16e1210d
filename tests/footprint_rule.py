"""Camera rays, ray differentials and texture footprints of ray-query hits as a rule in numpy float64 (rules F1-F8).  TEST INFRASTRUCTURE.

`camera_ray_kernel` and `hit_footprint_kernel` (csrc/footprint.hip) run the frame's device functions (primary_ray, compute_ray_diffs, inst_view, get_vertex_data
of csrc/shade.h) and restate its gradient block and the head of tex_sample_grad.  This module states the same operations from their meaning, on top of
tests/sampler_rule.py (primary_rays, ray_diffs, texture_grads, raw_lod / clamp_lod: imported, and reproduced here where this rule says more -- a jitter, a
render size that is not the screen size, a differential origin, a direction that is not normalised), and carries with every value a first-order bound on what a
float32 evaluation may differ by: the `F` arithmetic of tests/light_rule.py, as tests/surface_rule.py uses it.  It reads a `SceneData`, the sizes and level counts
of the textures, rays, differentials and hits; it imports nothing from oracle/ and nothing from the library.

Decisions.  A lod has three: rho > 0 (F7's first comparison), the clamp's ends 0 and mips - 1, and -- for an instance drawn under a POINT sampler, where each fetch
of the frame takes one level -- the level (int)(lod + 0.5) (`point_level`, applied to every fetch the frame makes).  Where the margin of one of them is below
DECISION_K x the bound of the quantity compared, the hit is *undecided*: it is compared up to both choices and counted.  A record carries lods, no level: the
level compared is the one the record's float32 lod selects (`compare_levels`).  A hit F8 calls degenerate (a bound that is not finite) is counted with them.

The lod's bound.  tests/test_gpu_sampler.py derives DLOD = 2^-12 for a frame's camera rays whose projection onto the surface amplifies by 1 / |cos| <= 16: some
60 float32 operations at 2^-24, times 16, over ln 2.  Here the same chain is walked operation by operation in `F`, so the bound of a steeper hit, of a differential
origin that cancels against t dD, or of a sliver triangle grows with the amplification it actually has; tests/test_footprint_rule.py asserts that on camera rays
with 1 / |cos| <= 16 the walked bound stays below DLOD, i.e. that the two derivations agree where both apply.
"""
import math

import numpy as np

import light_rule as L
import sampler_rule as SR
import surface_rule as S
from light_rule import F

VALID, BAD_HIT, HAS_UV, TEXTURED = 0x01, 0x02, 0x04, 0x08
DECISION_K = L.DECISION_K
DLOD = 2.0 ** -12                 # tests/test_gpu_sampler.py's bound of a camera ray's lod at 1 / |cos| <= 16
AMPLIFICATION = 16.0
RAY_MIN_DISTANCE, RAY_MAX_DISTANCE = float(np.float32(0.1)), 100000.0
MAX_MIPS = 16
PROJ_K = 8                        # float32 roundings in front of an entry of projectionI: tan (2 ulp), aspect, two quotients, the inverse's own rounding
CAMERA_K = L.CAM_K                # ... in front of a component of cameraU / V / W (an inverse, two normalisations, a cross product, tan, two products)
JITTER_K = 4                      # ... of a Halton value (a quotient and a sum per digit, at most three digits matter) minus 0.5
SHADER_NORMAL_MAP, SHADER_SPECULAR_MAP = 0x4, 0x8

MUTATIONS = ("jitter_left_out", "render_size_for_screen", "dDdy_sign", "direction_normalised", "dO_ignored", "object_space_corners", "detail_scale_not_applied",
             "diffuse_size_for_normal_map", "quirk_repaired", "mean_of_extents", "clamp_before_positive_test")


# ---- F2 / F3: the camera ray of a pixel ------------------------------------------------------------------------------------------------------------

def halton(index, base):
    """The radical inverse of `index` in `base` (tests/golden/kats.json pins the sequence)."""
    f, r, i = 1.0, 0.0, int(index)
    while i > 0:
        f /= base; r += f * (i % base); i //= base
    return r


def upscaler_jitter(frame, phases):
    """The jitter of frame `frame` (0 for the first) under an active upscaler: Halton(frame mod phases + 1, 2 / 3) - 0.5."""
    i = int(frame) % int(phases) + 1
    return halton(i, 2) - 0.5, halton(i, 3) - 0.5


def camera(data, screen_w, screen_h, render_w=None, render_h=None, jitter=(0.0, 0.0)):
    """What F2 / F3 read of a drawn frame: the view of `data`, the screen size (aspect, compute_ray_diffs), the render size (pixel -> NDC) and the jitter."""
    return dict(view=np.asarray(data.view, dtype=np.float32).astype(np.float64), fov=float(data.fov), near=float(data.near), far=float(data.far),
                screen=(int(screen_w), int(screen_h)), render=(int(render_w or screen_w), int(render_h or screen_h)), jitter=(float(jitter[0]), float(jitter[1])))


def _inverse4(m):
    """inverse of a float32 matrix as the host makes it (cofactors in double, each entry rounded to float32 once): 4 x 4 F."""
    inv = np.linalg.inv(m)
    err = L.U * np.abs(inv) + 4 * S.INVERSE_OPS * S.D * (np.abs(inv) @ np.abs(m) @ np.abs(inv))
    return [[F(inv[r, c], err[r, c]) for c in range(4)] for r in range(4)]


def camera_rays(cam, pixels, mutate=None):
    """F2 / F3 for (N, 2) integer pixels (any integers: outside the frame the rule extrapolates).  -> dict(origin, direction, dDdx, dDdy), each a (value, bound) pair of
    (N, 3) float64; dOdx = dOdy = 0, tMin = 0.1, tMax = 100000."""
    assert mutate is None or mutate in MUTATIONS, mutate
    px = np.asarray(pixels, dtype=np.int64).reshape(-1, 2).astype(np.float64)
    sw, sh = cam["screen"]; rw, rh = cam["render"]
    jx, jy = (0.0, 0.0) if mutate == "jitter_left_out" else cam["jitter"]
    jit = [F(j, JITTER_K * L.U * abs(j)) for j in (jx, jy)]
    ndc = [L.sub(L.mul(L.div(L.add(F(px[:, k] + 0.5), jit[k]), float(n)), 2.0), 1.0) for k, n in ((0, rw), (1, rh))]
    aspect = sw / sh
    h = 1.0 / math.tan(0.5 * cam["fov"])
    pa, pb = aspect / h, 1.0 / h                                           # projectionI[0][0], [1][1]; [3][2] is -1 exactly, [2][2] is 0
    target = [L.mul(ndc[0], F(pa, PROJ_K * L.U * pa)), L.mul(L.neg(ndc[1]), F(pb, PROJ_K * L.U * pb)), F(np.full(len(px), -1.0))]
    vi = _inverse4(cam["view"])
    direction = [L.add(L.add(L.mul(target[0], vi[0][c]), L.mul(target[1], vi[1][c])), L.mul(target[2], vi[2][c])) for c in range(3)]
    if mutate == "direction_normalised":          # (F5's projection itself does not see the length of the direction; the ray, its t and with t the differential's reach do)
        direction = L.normalize3(direction)
    origin = [F(np.full(len(px), vi[3][c].v), vi[3][c].e) for c in range(3)]
    Uv, Vv, Wv = SR.camera_vectors(cam["view"], cam["fov"], cam["near"], cam["far"], aspect)
    cu, cv, cw = ([F(x[c], CAMERA_K * L.U * np.linalg.norm(x)) for c in range(3)] for x in (Uv, Vv, Wv))
    non_norm = [L.add(L.add(L.mul(cu[c], ndc[0]), L.mul(cv[c], ndc[1])), cw[c]) for c in range(3)]
    vw, vh = (rw, rh) if mutate == "render_size_for_screen" else (sw, sh)
    dd = L.dot3(non_norm, non_norm)
    divd = L.div(2.0, L.mul(dd, L.sqrt(dd)))
    dr, du = L.dot3(non_norm, cu), L.dot3(non_norm, cv)
    dDdx = [L.mul(L.mul(L.sub(L.mul(cu[c], dd), L.mul(non_norm[c], dr)), divd), L.rcp(F(float(vw)))) for c in range(3)]
    dDdy = [L.neg(L.mul(L.mul(L.sub(L.mul(cv[c], dd), L.mul(non_norm[c], du)), divd), L.rcp(F(float(vh))))) for c in range(3)]
    if mutate == "dDdy_sign":
        dDdy = L.neg3(dDdy)
    return {k: S._stack(v) for k, v in (("origin", origin), ("direction", direction), ("dDdx", dDdx), ("dDdy", dDdy))}


def as_rays(rule):
    """The rule's camera rays and differentials as the float32 arrays the calls return: (N, 8) RT64_RAYs and (N, 16) RT64_RAY_DIFFERENTIALs."""
    n = len(rule["origin"][0])
    rays = np.zeros((n, 8), dtype=np.float32); diffs = np.zeros((n, 16), dtype=np.float32)
    rays[:, 0:3] = rule["origin"][0]; rays[:, 3] = RAY_MIN_DISTANCE; rays[:, 4:7] = rule["direction"][0]; rays[:, 7] = RAY_MAX_DISTANCE
    diffs[:, 8:11] = rule["dDdx"][0]; diffs[:, 12:15] = rule["dDdy"][0]
    return rays, diffs


def compare_rays(rule, rays, diffs):
    """Largest |array - rule| / bound of origin, direction, dDdx, dDdy; and whether tMin, tMax, dOdx, dOdy and the reserved words are exactly F2 / F3's."""
    rays = np.asarray(rays, dtype=np.float32); diffs = np.asarray(diffs, dtype=np.float32)
    ratios = {}
    for name, got in (("origin", rays[:, 0:3]), ("direction", rays[:, 4:7]), ("dDdx", diffs[:, 8:11]), ("dDdy", diffs[:, 12:15])):
        d = np.abs(got.astype(np.float64) - rule[name][0])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d == 0.0, 0.0, d / rule[name][1])
        ratios[name] = np.where(np.isnan(r), np.inf, r).max(axis=1)
    exact = (rays[:, 3] == np.float32(0.1)) & (rays[:, 7] == np.float32(100000.0)) & ~diffs.view(np.uint32)[:, [0, 1, 2, 3, 4, 5, 6, 7, 11, 15]].any(axis=1)
    return ratios, exact


# ---- F4 - F8: the footprint of a hit ----------------------------------------------------------------------------------------------------------------

def mip_count(w, h):
    """Levels of a generated chain (mipgen rule M2)."""
    return min(int(math.floor(math.log2(max(w, h)))) + 1, MAX_MIPS)


def texture_table(data, levels=None, generated=False):
    """texture index -> (width, height, mips): from read-back levels (index -> list of arrays), or from the scene's RGBA8 images with one level each
    (generated: a whole chain)."""
    out = {}
    for k, t in enumerate(data.textures):
        if levels is not None and k in levels:
            out[k] = (levels[k][0].shape[1], levels[k][0].shape[0], len(levels[k]))
        elif t.format == 0x1:
            out[k] = (int(t.width), int(t.height), mip_count(t.width, t.height) if generated else 1)
    return out


def shader_of(data, inst):
    """(shaderId, flags, filter) an instance is drawn with."""
    if inst.shader is not None:
        return int(inst.shader[0]), int(inst.shader[4]), int(inst.shader[1])
    return int(data.shader_id), int(data.shader_flags), int(data.shader_filter)


def combiner_reads(shader_id):
    """(reads texel 0, layout has a UV): slots 5 / 6 name texel 0, slot 7 texel 1, in either cycle."""
    slots = [(shader_id >> (3 * i)) & 7 for i in range(8)]
    return any(s in (5, 6) for s in slots), any(s in (5, 6, 7) for s in slots)


def lod_of(ddx, ddy, size, mutate=None):
    """F7 for one texture: ddx, ddy two F each (the gradients this texture's fetch is handed), size = (width, height, mips).  -> dict(lod: the clamped value, bound,
    raw: log2 rho, low / high: the clamp decides for 0 / mips - 1, undecided, rho: F)."""
    w0, h0, mips = size
    ax, ay, bx, by = L.mul(ddx[0], float(w0)), L.mul(ddx[1], float(h0)), L.mul(ddy[0], float(w0)), L.mul(ddy[1], float(h0))
    with np.errstate(invalid="ignore", over="ignore"):
        ea, eb = L.sqrt(L.add(L.mul(ax, ax), L.mul(ay, ay))), L.sqrt(L.add(L.mul(bx, bx), L.mul(by, by)))
        if mutate == "mean_of_extents":
            rho = L.mul(L.add(ea, eb), 0.5)
        else:                                        # fmax: a NaN side loses
            va = np.where(np.isnan(ea.v), -np.inf, ea.v); vb = np.where(np.isnan(eb.v), -np.inf, eb.v)
            both = np.isnan(ea.v) & np.isnan(eb.v)
            rho = F(np.where(both, np.nan, np.maximum(va, vb)), np.where(both, np.nan, np.maximum(np.where(np.isnan(ea.e), 0.0, ea.e), np.where(np.isnan(eb.e), 0.0, eb.e))))
        positive = rho.v > 0.0                       # (false for a NaN)
        safe = np.where(positive, rho.v, 1.0)
        raw = np.where(positive, np.log2(safe), -np.inf)
        lo = safe - rho.e
        e = np.where(positive & (lo > 0.0), rho.e / (np.where(lo > 0.0, lo, 1.0) * math.log(2.0)) + np.maximum(L.A * np.abs(raw), L.LOG_FLOOR), np.inf)
        e = np.where(positive, e, np.where(np.isfinite(rho.e) & (rho.e == 0.0), 0.0, np.inf))          # rho = 0 exactly (zero gradients): the lod is 0, no doubt about it
    max_lod = float(mips - 1)
    if mutate == "clamp_before_positive_test":
        # the clamp taken first, as min / max that hand a NaN on, and on log2 of whatever rho is; the test for rho > 0 then finds a NaN neither positive nor not
        with np.errstate(invalid="ignore", divide="ignore"):
            lod = np.clip(np.log2(rho.v), 0.0, max_lod)
    else:
        lod = np.where(raw > 0.0, np.minimum(raw, max_lod), 0.0)
    if mips == 1:
        return dict(lod=np.zeros_like(lod) if mutate != "clamp_before_positive_test" else lod * 0.0, bound=np.zeros_like(lod), raw=raw, low=np.ones(lod.shape, dtype=bool),
                    high=np.zeros(lod.shape, dtype=bool), undecided=np.zeros(lod.shape, dtype=bool), rho=rho)
    with np.errstate(invalid="ignore"):
        margin = DECISION_K * e
        rho_doubt = ~np.isnan(rho.v) & (rho.e > 0.0) & (np.abs(rho.v) <= DECISION_K * rho.e)
        undecided = rho_doubt | (positive & ((np.abs(raw) < margin) | (np.abs(raw - max_lod) < margin)))
        undecided |= positive & ~np.isfinite(e)
        low = ~undecided & ~(raw > 0.0)
        high = ~undecided & (raw > max_lod)
    return dict(lod=lod, bound=np.where(low | high, 0.0, e), raw=raw, low=low, high=high, undecided=undecided, rho=rho)


def point_level(lod, bound):
    """The level a POINT sampler takes at `lod`, (int)(lod + 0.5), and whether the lod lies within DECISION_K x its bound of a half-integer (a bound that is not
    finite leaves every level open)."""
    lod = np.asarray(lod, dtype=np.float64)
    frac = (lod + 0.5) - np.floor(lod + 0.5)
    with np.errstate(invalid="ignore"):
        return np.floor(lod + 0.5).astype(np.int64), ~(np.minimum(frac, 1.0 - frac) >= DECISION_K * np.asarray(bound, dtype=np.float64))


def compare_levels(rule, got):
    """Under a POINT sampler the level a record's lod selects, (int)(lod + 0.5) of the float32 the device wrote, against the rule's: equal on every fetch whose level
    is decided, one of the two levels next to the rule's lod where it is not.  -> ok [N] (True where no fetch is POINT), and how many fetches were compared."""
    got = np.asarray(got, dtype=np.float32)
    ok = np.ones(len(got), dtype=bool); compared = 0
    real = rule["kind"] == 2
    for name, col in (("lod", 4), ("lod_normal", 5), ("lod_specular", 6)):
        r = rule[name]
        m = real & r["taken"] & r["point"] & ~rule["degenerate"] & ~r["undecided"]
        dev = np.floor(got[:, col].astype(np.float64) + 0.5).astype(np.int64)
        near = (dev == np.floor(r["lod"]).astype(np.int64)) | (dev == np.ceil(r["lod"]).astype(np.int64))
        ok &= np.where(m, np.where(r["level_undecided"], near, dev == r["level"]), True)
        compared += int(m.sum())
    return ok, compared


def footprints(data, textures, rays, diffs, hits, mutate=None):
    """F4-F8.  textures: texture_table().  rays, hits (N, 8) float32; diffs (N, 16) float32 or None.  -> dict of per-record arrays: kind (0 miss, 1 bad hit, 2 real),
    duv (value, bound) (N, 4): duvdx xy, duvdy xy; dP (value, bound) (N, 6): dPdx xyz, dPdy xyz; lod / lod_normal / lod_specular: lod_of() dicts scattered to N
    (taken: the frame makes that fetch; point / level / level_undecided: under a POINT sampler the level (int)(lod + 0.5) that fetch takes, and whether the lod
    lies within its bound of a half-integer); has_uv, textured, undecided, degenerate (bool), amplification (1 / |cos| of direction and triangle normal), instance,
    primitive."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rays = np.asarray(rays, dtype=np.float32); hits = np.asarray(hits, dtype=np.float32)
    n = len(rays)
    diffs = np.zeros((n, 16), dtype=np.float32) if diffs is None else np.asarray(diffs, dtype=np.float32)
    hi = hits.view(np.int32); hu = hits.view(np.uint32)
    inst = hi[:, 3].astype(np.int64); prim = hu[:, 4].astype(np.int64)
    rt = S.raytraced_instances(data)
    out = {"kind": np.zeros(n, dtype=np.int64), "instance": inst, "primitive": prim, "amplification": np.zeros(n)}
    for k in ("has_uv", "textured", "undecided", "degenerate"):
        out[k] = np.zeros(n, dtype=bool)
    out["duv"] = (np.zeros((n, 4)), np.zeros((n, 4))); out["dP"] = (np.zeros((n, 6)), np.zeros((n, 6)))
    for k in ("lod", "lod_normal", "lod_specular"):
        out[k] = dict(lod=np.zeros(n), bound=np.zeros(n), raw=np.full(n, -np.inf), low=np.zeros(n, dtype=bool), high=np.zeros(n, dtype=bool),
                      undecided=np.zeros(n, dtype=bool), taken=np.zeros(n, dtype=bool), mips=np.ones(n, dtype=np.int64),
                      point=np.zeros(n, dtype=bool), level=np.zeros(n, dtype=np.int64), level_undecided=np.zeros(n, dtype=bool))
    out["kind"][inst >= 0] = 1
    for k, index in enumerate(rt):
        I = data.instances[index]
        mesh = data.meshes[I.mesh]
        sel = np.nonzero((inst == k) & (prim < len(mesh.indices) // 3))[0]
        if not len(sel):
            continue
        out["kind"][sel] = 2
        shader_id, shader_flags, shader_filter = shader_of(data, I)
        layout = S.vertex_layout(shader_id)
        tex0, has_uv = combiner_reads(shader_id)
        assert has_uv == layout["has_uv"]
        corner = [np.asarray(mesh.indices, dtype=np.int64)[3 * prim[sel] + c] for c in range(3)]
        p = [S._fetch(mesh, layout, corner[c], 0, 3) for c in range(3)]
        T = np.asarray(I.transform, dtype=np.float32).astype(np.float64)
        pF = [S._vecF(x) for x in p]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            tn = L.neg3(L.cross3(L.sub3(pF[2], pF[0]), L.sub3(pF[1], pF[0])))
            N = L.normalize3(S._mul_vector(S._normal_matrix(T), tn))
            D = S._vecF(rays[sel, 4:7].astype(np.float64))          # as given: F5's projection does not change with its length, t does -- it counts in units of it
            t = F(hits[sel, 0].astype(np.float64))
            dO = [S._vecF(diffs[sel, 0:3].astype(np.float64)), S._vecF(diffs[sel, 4:7].astype(np.float64))]
            dD = [S._vecF(diffs[sel, 8:11].astype(np.float64)), S._vecF(diffs[sel, 12:15].astype(np.float64))]
            DN = L.dot3(D, N)
            rcpDN = L.rcp(DN)
            dP = []
            for a in range(2):                                    # F5
                o = L.scale3(dD[a], t) if mutate == "dO_ignored" else L.add3(dO[a], L.scale3(dD[a], t))
                dt = L.mul(L.neg(L.dot3(o, N)), rcpDN)
                dP.append(L.add3(o, L.scale3(D, dt)))
            v, e = S._stack(dP[0] + dP[1])
            out["dP"][0][sel], out["dP"][1][sel] = v, e
            dlen = np.linalg.norm(rays[sel, 4:7].astype(np.float64), axis=1)
            out["amplification"][sel] = np.where(DN.v != 0.0, dlen / np.abs(np.where(DN.v != 0.0, DN.v, 1.0)), np.inf)
            degenerate = ~np.isfinite(e).all(axis=1) | ~np.isfinite(v).all(axis=1)
            zero = [F(np.zeros(len(sel))), F(np.zeros(len(sel)))]
            grads = [zero, zero]
            if has_uv:                                            # F6
                out["has_uv"][sel] = True
                corners = pF if mutate == "object_space_corners" else [
                    [L.add(L.add(L.add(L.mul(q[0], T[0, c]), L.mul(q[1], T[1, c])), L.mul(q[2], T[2, c])), T[3, c]) for c in range(3)] for q in pF]
                e01, e02 = L.sub3(corners[1], corners[0]), L.sub3(corners[2], corners[0])
                Nu, Nv = L.cross3(e02, N), L.cross3(e01, N)
                Lu, Lv = L.scale3(Nu, L.rcp(L.dot3(Nu, e01))), L.scale3(Nv, L.rcp(L.dot3(Nv, e02)))
                uv = [S._fetch(mesh, layout, corner[c], layout["uv"], 2) for c in range(3)]
                uv01 = [L.sub(F(uv[1][:, c]), F(uv[0][:, c])) for c in range(2)]; uv02 = [L.sub(F(uv[2][:, c]), F(uv[0][:, c])) for c in range(2)]
                grads = []
                for a in range(2):
                    bx, by = L.dot3(Lu, dP[a]), L.dot3(Lv, dP[a])
                    grads.append([L.add(L.mul(bx, uv01[c]), L.mul(by, uv02[c])) for c in range(2)])
                v, e = S._stack(grads[0] + grads[1])
                out["duv"][0][sel], out["duv"][1][sel] = v, e
                degenerate |= ~np.isfinite(e).all(axis=1) | ~np.isfinite(v).all(axis=1)
            out["degenerate"][sel] = degenerate
            # F7: what the frame hands each fetch
            textured = tex0 and has_uv
            out["textured"][sel] = textured
            handed = grads if (textured or mutate == "quirk_repaired") else [zero, zero]
            s = float(np.float32(I.material.uvDetailScale))
            scaled = [[L.mul(g, s) for g in handed[a]] for a in range(2)]
            fetches = [("lod", textured, I.diffuse, handed, I.diffuse)]
            fetches.append(("lod_normal", has_uv and bool(shader_flags & SHADER_NORMAL_MAP) and I.normal is not None, I.normal,
                            handed if mutate == "detail_scale_not_applied" else scaled, I.diffuse if mutate == "diffuse_size_for_normal_map" else I.normal))
            fetches.append(("lod_specular", has_uv and bool(shader_flags & SHADER_SPECULAR_MAP) and I.specular is not None, I.specular, scaled, I.specular))
            und = np.zeros(len(sel), dtype=bool)
            for key, taken, _, g, sized in fetches:
                if not taken:
                    continue
                r = lod_of(g[0], g[1], textures[sized], mutate)
                for f in ("lod", "bound", "raw", "low", "high", "undecided"):
                    out[key][f][sel] = r[f]
                out[key]["taken"][sel] = True; out[key]["mips"][sel] = textures[sized][2]
                und |= r["undecided"]
                if shader_filter == SR.POINT:                     # the third decision: the level this fetch of the frame takes at its lod
                    level, doubt = point_level(r["lod"], r["bound"])
                    doubt &= textures[sized][2] > 1               # (a one-level texture has no other level to take)
                    out[key]["point"][sel] = True; out[key]["level"][sel] = level; out[key]["level_undecided"][sel] = doubt
                    und |= doubt
            out["undecided"][sel] = und | degenerate
    return out


def as_records(rule):
    """The rule's own values in RT64_RAY_FOOTPRINT's layout, (N, 16) float32."""
    n = len(rule["kind"])
    rec = np.zeros((n, 16), dtype=np.float32); ri = rec.view(np.uint32)
    real = rule["kind"] == 2
    with np.errstate(invalid="ignore", over="ignore"):
        rec[:, 0:4] = rule["duv"][0]; rec[:, 8:11] = rule["dP"][0][:, 0:3]; rec[:, 12:15] = rule["dP"][0][:, 3:6]
        rec[:, 4] = rule["lod"]["lod"]; rec[:, 5] = rule["lod_normal"]["lod"]; rec[:, 6] = rule["lod_specular"]["lod"]
    ri[:, 7] = np.where(real, VALID | np.where(rule["has_uv"], HAS_UV, 0) | np.where(rule["textured"], TEXTURED, 0), np.where(rule["kind"] == 1, BAD_HIT, 0))
    ri[:, 11] = np.where(real, rule["instance"], -1).astype(np.int64) & 0xFFFFFFFF
    ri[:, 15] = np.where(real, rule["primitive"], 0xFFFFFFFF)
    return rec


def compare(rule, got):
    """Per record: ratio |record - rule| / bound of the gradients and of dPd* on hits that are not degenerate (the largest over the components; a NaN counts as inf);
    ratio of the three lods where the clamp does not decide, and `lods_ok`: finite, inside [0, mips - 1], exactly 0 or mips - 1 where the rule says the clamp decides,
    exactly 0 where the frame makes no such fetch, anywhere between the two choices where the hit is undecided; `exact`: flags, instance, primitive the rule's, and a
    record that is no real hit equal to the miss / bad-hit record word for word."""
    got = np.asarray(got, dtype=np.float32); gi = got.view(np.uint32)
    want = as_records(rule); wi = want.view(np.uint32)
    real = rule["kind"] == 2
    exact = (gi[:, 7] == wi[:, 7]) & (gi[:, 11] == wi[:, 11]) & (gi[:, 15] == wi[:, 15])
    exact &= real | (gi == wi).all(axis=1)
    ratios = {}
    compared = real & ~rule["degenerate"]
    for name, cols, (v, e) in (("duv", [0, 1, 2, 3], rule["duv"]), ("dP", [8, 9, 10, 12, 13, 14], rule["dP"])):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            d = np.abs(got[:, cols].astype(np.float64) - v)
            r = np.where(d == 0.0, 0.0, d / e)
        ratios[name] = np.where(compared, np.where(np.isnan(r), np.inf, r).max(axis=1), 0.0)
    lods_ok = np.ones(len(real), dtype=bool)
    for name, col in (("lod", 4), ("lod_normal", 5), ("lod_specular", 6)):
        r = rule[name]; g = got[:, col].astype(np.float64)
        top = (r["mips"] - 1).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = np.isfinite(g) & (g >= 0.0) & (g <= top)
            ok &= np.where(real & r["taken"], True, g == 0.0)
            ok &= np.where(r["low"] & r["taken"] & real, g == 0.0, True) & np.where(r["high"] & r["taken"] & real, g == top, True)
            decided = real & r["taken"] & ~r["undecided"] & ~r["low"] & ~r["high"] & ~rule["degenerate"]
            d = np.abs(g - r["lod"])
            q = np.where(d == 0.0, 0.0, d / r["bound"])
        ratios[name] = np.where(decided, np.where(np.isnan(q), np.inf, q), 0.0)
        lods_ok &= ok
    return ratios, exact, lods_ok


def report(name, rule, ratios, exact, lods_ok):
    """One line per case, laid out like profiles/lighting_rule_deviation.txt."""
    real = rule["kind"] == 2
    n = int(real.sum())
    parts = ["%-34s hits %5d of %5d" % (name, n, len(real))]
    for k in ("duv", "dP", "lod", "lod_normal", "lod_specular"):
        r = ratios[k][real]
        parts.append("%s max %.3f mean %.4f" % (k, r.max() if n else 0.0, r.mean() if n else 0.0))
    parts.append("undecided %.4f" % (float(rule["undecided"][real].mean()) if n else 0.0))
    parts.append("inexact %d" % int((~exact).sum() + (~lods_ok).sum()))
    return "  ".join(parts)
