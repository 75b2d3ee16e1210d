"""The radiance queries (RT64_SkyViewRays, RT64_SkyViewPixels, RT64_ComposeViewRayRadiance, RT64_TraceViewRayRadiance, include/rt64_radiance.h) on the GPU, held to
the float64 rule of tests/radiance_rule.py ray by ray (the independent check), to the library's other ray-query calls -- the sentence of rt64_layers.h, `picture = sum of weights x what each layer shows + transmittance x background`, recomputed
from their records (rules W3-W7) -- and to themselves: the forms agree byte for byte, with and without the LDS scene cache, the composite call is
the two steps, maxLayers = m is the first m layers of 16, nothing is written past the last record and every slot before it is, bad records and bad calls are
answered as W3 and W10 say, and frames do not notice.

One run's lines of the rule test, the composition test and the sky test are committed as profiles/radiance_rule_deviation.txt.
"""
import copy

import numpy as np
import pytest

import layers_cases as LC
import layers_rule as LR
import material_cases as MC
import radiance_cases as RC
import ray_rule

pytestmark = pytest.mark.gpu

W, H = RC.W, RC.H
CULL = ray_rule.CULL_BACK_FACING
GUARD = 0xABABABAB
U = 2.0 ** -24
EPSILON = float(np.float32(1e-6))
F32 = np.float32


def _open(rt64_lib, data, options=None, w=W, h=H):
    from sm64rt_legacy_renderer_amd import sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, data, w, h, hip_device=0)
    for k, v in (options or {}).items():
        assert s.option(k, v), k
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _unorm8(x):
    """q_unorm8 of device_math.h in float32: 0 unless x > 0, 1 from 1 on, else floor(x 255 + 0.5) / 255."""
    x = np.asarray(x, dtype=np.float32)
    k = np.floor(x * F32(255.0) + F32(0.5)).astype(np.float32)
    k = np.where(x > 0, np.where(x >= 1, F32(255.0), k), F32(0.0)).astype(np.float32)
    return (k / F32(255.0)).astype(np.float32)


def compose(rt64_lib, view, data, rays, lods, flags):
    """W3-W7 from the records of the existing calls, in float64 on their float32 values: the list and its weights (RT64_TraceViewRayLayers with weights), each layer's
    colour (RT64_ShadeViewRayHits, rounded to UNORM8 as the frame stores it), the light at litLayer (RT64_LightViewRayHits: `direct` or `unshadowed`; `emitted` minus the
    eye light is the instance's selfLight, taken from the scene), the sky (RT64_SkyViewRays).  Fog is W5's, restated here from the material.  -> dict of value arrays
    `mag` (per field, the sum of the magnitudes of its terms: what a float32 evaluation's roundings are proportional to) and `slack` (see ROUNDINGS)."""
    from sm64rt_legacy_renderer_amd import rt64
    import surface_rule as S
    n = len(rays)
    hits, layers, weights, coverage = rt64.trace_view_ray_layers(rt64_lib, view, rays, 16, lods, weights=True)
    sky = rt64.sky_view_rays(rt64_lib, view, rays).astype(np.float64)[:, :3]
    rt = S.raytraced_instances(data)
    mats = [data.instances[i].material for i in rt]
    tab = lambda f: np.array([f(m) for m in mats], dtype=np.float64)
    mask = np.array([int(m.lightGroupMaskBits) for m in mats], dtype=np.int64)
    self_light = tab(lambda m: (F32(m.selfLight.x), F32(m.selfLight.y), F32(m.selfLight.z)))
    fog_on = np.array([int(m.fogEnabled) for m in mats], dtype=np.int64)
    fog_colour = tab(lambda m: (F32(m.fogColor.x), F32(m.fogColor.y), F32(m.fogColor.z)))
    fog_mul, fog_offset, bias = tab(lambda m: F32(m.fogMul)), tab(lambda m: F32(m.fogOffset)), tab(lambda m: F32(m.depthBias))
    d = data.desc
    ambient = np.array([F32(F32(getattr(d.ambientBaseColor, c)) + F32(getattr(d.ambientNoGIColor, c))) for c in "xyz"], dtype=np.float64)
    o64, d64 = (np.nan_to_num(rays[:, c:c + 3].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) for c in (0, 4))          # (a Q6-invalid ray has no layer)
    surface, transparent = np.zeros((n, 3)), np.zeros((n, 3))
    mag = {"surface": np.zeros((n, 3)), "transparent": np.zeros((n, 3))}          # the sums of the terms' magnitudes
    slack = np.zeros((n, 3))          # what the fog alpha's own float32 error moves `transparent` and `surface` by (see ROUNDINGS)
    lit = np.full(n, -1, dtype=np.int64); shaded = np.zeros(n, dtype=np.int64); fogged = np.zeros(n, dtype=bool)
    near_gate = np.zeros(n, dtype=bool)
    vp = _view_proj(data)
    for l in range(16):
        inst = _bits(hits[l])[:, 3].view(np.int32).astype(np.int64)
        w = weights[l].astype(np.float64)
        on = w > 0.0                                                          # T7: a layer with a weight; behind the list's end and behind coverage the weight is 0
        if not on.any():
            continue
        mat = rt64.shade_hits(rt64_lib, view, rays, hits[l], lods)
        colour = _unorm8(mat[:, :4]).astype(np.float64)
        k = np.where(on, inst, 0)
        t = np.where(on, hits[l][:, 0], F32(0.0)).astype(np.float64)
        reach = (t - bias[k]) + bias[k]
        pos = o64 + d64 * reach[:, None]
        pos_e = 4.0 * U * (np.abs(o64) + np.abs(d64) * np.abs(reach)[:, None])          # the float32 position: a product and a sum per component, and the rounding of `reach`
        f = on & (fog_on[k] != 0)
        if flags & rt64.RADIANCE_FLAG_FOG_FROM_CAMERA:
            p4 = np.concatenate([pos, np.ones((n, 1))], axis=1)
            clip = p4 @ vp
            clip_e = np.concatenate([pos_e, np.zeros((n, 1))], axis=1) @ np.abs(vp) + 8.0 * U * (np.abs(p4) @ np.abs(vp))
            z = clip[:, 2] * 2.0 - clip[:, 3]
            wc = np.maximum(clip[:, 3], float(F32(0.001)))
            q = z / wc
            q_e = (2.0 * clip_e[:, 2] + clip_e[:, 3]) / wc + np.abs(q) * clip_e[:, 3] / wc
            raw = (q * fog_mul[k] + fog_offset[k]) / 255.0
            fa_e = q_e * np.abs(fog_mul[k]) / 255.0
        else:
            raw = ((np.linalg.norm(pos - o64, axis=1) + fog_offset[k]) / fog_mul[k]) * 0.5
            fa_e = np.linalg.norm(pos_e, axis=1) / np.abs(fog_mul[k]) * 0.5
        raw, fa_e = np.where(f, raw, 0.0), np.where(f, fa_e, 0.0)
        near_gate |= f & ((np.abs(raw) < 4.0 * fa_e + 1e-6) | (np.abs(raw - 1.0) < 4.0 * fa_e + 1e-6))          # at a clamp end of the fog alpha float32 may land on the other side
        fa = np.clip(raw, 0.0, 1.0)
        fa_e = np.where((raw > 0.0) & (raw < 1.0), fa_e, 0.0)                     # clamped, and decidedly so: exact
        fog_term = np.where(f[:, None], fog_colour[k] * (fa * w)[:, None], 0.0)
        transparent += fog_term; mag["transparent"] += np.abs(fog_term)
        wf = w * (1.0 - fa)
        lit_layer = on & (mask[k] > 0)
        add = np.where(on[:, None], colour[:, :3] * wf[:, None], 0.0)
        surface += np.where(lit_layer[:, None], add, 0.0); mag["surface"] += np.where(lit_layer[:, None], add, 0.0)
        unlit = np.where((on & ~lit_layer)[:, None], add * (ambient[None] + self_light[k]), 0.0)
        transparent += unlit; mag["transparent"] += np.abs(unlit)
        slack += (w * fa_e)[:, None] * np.maximum(np.abs(fog_colour[k]), np.maximum(colour[:, :3], colour[:, :3] * np.abs(ambient[None] + self_light[k])))
        lit = np.where(on, l, lit); shaded += on; fogged |= f
    rem = coverage[:, 0].astype(np.float64)                                  # T7's transmittance: the same float32 operations
    light, direct = np.zeros((n, 3)), np.zeros((n, 3), dtype=np.float32)
    has = lit >= 0
    if has.any():
        at = np.ascontiguousarray(hits[np.maximum(lit, 0), np.arange(n)])
        lr = rt64.light_hits(rt64_lib, view, rays, at, lods)
        k = np.where(has, _bits(at)[:, 3].view(np.int32).astype(np.int64), 0)
        direct = lr[:, 4:7] if flags & rt64.RADIANCE_FLAG_UNSHADOWED else lr[:, 0:3]
        light = np.where(has[:, None], ambient[None] + (direct.astype(np.float64) + self_light[k]), 0.0)
    radiance = np.where(has[:, None], surface * light, surface)
    mag["light"] = np.abs(light)
    mag["radiance"] = np.where(has[:, None], mag["surface"] * np.abs(light), mag["surface"]) + np.abs(sky) * rem[:, None] + mag["transparent"]
    slack_of = {"surface": slack, "transparent": slack, "light": np.zeros((n, 3)), "radiance": slack * np.maximum(1.0, np.abs(light))}
    valid = (_bits(coverage)[:, 3] & LR.COVERAGE_VALID) != 0
    radiance = np.where(valid[:, None], radiance + (sky * rem[:, None] + transparent), 0.0)
    return dict(radiance=radiance, surface=surface, transparent=transparent, light=light, lit=lit, shaded=shaded, fogged=fogged, coverage=coverage, layers=layers,
                mag=mag, slack=slack_of, near_gate=near_gate, direct=np.where(has[:, None], direct, 0.0), hits=hits, sky=sky, valid=valid)


def _view_proj(data):
    """view x projection (row vectors) from the float32 view matrix and the perspective the host builds from fov, near and far: the camera fog of W5 reads it."""
    sy = 1.0 / np.tan(0.5 * float(data.fov)); sx = sy / (W / H); rng = float(data.far) / (float(data.near) - float(data.far))
    proj = np.zeros((4, 4)); proj[0, 0] = sx; proj[1, 1] = sy; proj[2, 2] = rng; proj[2, 3] = -1.0; proj[3, 2] = rng * float(data.near)
    return np.asarray(data.view, dtype=np.float32).astype(np.float64) @ proj


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_records_lie_within_the_rule_ray_by_ray(rt64_lib, oracle_lib, sample_data, name):
    """1.  Per case, under both settings of UNSHADOWED (and, on fog_8, with the camera's fog): every decided ray's radiance, surface, transparent, light and
    transmittance within the bound of tests/radiance_rule.py, litLayer, layers and flags exact.  The mutations assigned to the case leave the device's records."""
    from sm64rt_legacy_renderer_amd import rt64
    import material_rule as M
    import radiance_rule as R
    from test_radiance_rule import MUTATION_CASES, scene_of
    data, rays, lods = scene_of(sample_data, name)
    settings = [0, rt64.RADIANCE_FLAG_UNSHADOWED] + ([rt64.RADIANCE_FLAG_FOG_FROM_CAMERA] if name == "fog_8" else [])
    s = _open(rt64_lib, data)
    try:
        s.draw()
        got = {f: rt64.trace_view_ray_radiance(rt64_lib, s.view, rays, 16, lods, flags=f, hits=False, layers=False) for f in settings}
    finally:
        s.close()
    levels = M.texture_levels(data)
    o, cand = LC.enumerate_candidates(data, rays)
    try:
        for f in settings:
            rule = R.radiance(data, levels, rays, cand, lods, f, R.sky_of(data, W, H), R.view_proj(data, W, H), oracle_scene=o)
            ratios, exact = R.compare(rule, got[f])
            print("rule %-10s flags %#05x  rays %3d  undecided %.4f  two or more layers %3d  misses %3d  fogged %3d  unlit last %3d  a light blocked %3d  discrete fields that differ %d  "
                  "ratio radiance %.3f surface %.3f transparent %.3f light %.3f transmittance %.3f" %
                  (name, f, len(rays), rule["undecided"].mean(), int((rule["layers"] >= 2).sum()), int((rule["valid"] & (rule["layers"] == 0)).sum()), int(rule["fogged"].sum()),
                   int(rule["unlit_last"].sum()), int(rule["shaded_by_walk"].sum()), int((~exact).sum()), *[float(ratios[k].max()) for k in ("radiance", "surface", "transparent", "light", "transmittance")]))
            assert rule["undecided"].mean() <= 0.005
            assert exact.all(), (name, f, np.nonzero(~exact)[0][:8].tolist())
            for k, r in ratios.items():
                assert (r <= 1.0).all(), (name, f, k, float(r.max()), np.nonzero(~(r <= 1.0))[0][:8].tolist())
            for mutation, (where, mflags) in MUTATION_CASES.items():
                if where != name or mflags != f:
                    continue
                wrong = R.radiance(data, levels, rays, cand, lods, f, R.sky_of(data, W, H), R.view_proj(data, W, H), oracle_scene=o, mutate=mutation)
                mr, me = R.compare(wrong, got[f])
                out = ~me | np.any([~(r <= 1.0) for r in mr.values()], axis=0)
                print("    mutation %-28s %4d of %4d of the device's rays outside it" % (mutation, int(out.sum()), len(out)))
                assert out.sum() >= 1, mutation
    finally:
        o.close()


# The bound of the composition identity.  Both sides start from the same float32 numbers: the layers' stored colours and weights, the lights' terms, the sky.  The device
# evaluates W5-W7 in float32, this test in float64; they differ by the device's own roundings only.  A term of `surface` or `transparent` is a product of at most five
# factors, a sum of up to 16 of them adds one rounding per layer, `light` is two sums, radiance one product and two sums: fewer than 32 roundings of 2^-24 each, relative to
# the sum of the magnitudes of the terms (`mag`).  The fog alpha is the one quantity the device computes from geometry rather than from a record: the float32 position
# origin + direction x reach is off by up to 4 x 2^-24 (|origin| + |direction| reach) per component, whatever the distance (or the clip-space quotient) made from it;
# `slack` carries that through (distance + offset) / mul / 2 -- or the camera's quotient -- times the layer's weight and colour.  A fog alpha within four such errors of a
# clamp end is not compared (near_gate).
ROUNDINGS = 32


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_record_is_the_composition_of_the_existing_calls(rt64_lib, sample_data, name):
    """2.  The sentence of rt64_layers.h, tested, and radiance.hip's layer colour and light held to the records of material.hip and lighting.hip more closely than the rule's bound
    can (the independent check is test 1; this one shares the library's own colours and lights): recomputed from RT64_TraceViewRayLayers' weights, RT64_ShadeViewRayHits per layer, RT64_LightViewRayHits at litLayer and
    RT64_SkyViewRays, transmittance and layers match bit for bit, litLayer and the flags exactly, and every colour within ROUNDINGS x 2^-24 of the terms' magnitudes --
    shadowed and UNSHADOWED, fog from the origin and (fog_8) from the camera."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K = RC.case(sample_data, name)
    rays = RC.rays_of(K, RC.SEEDS[name], name=name, data=data)
    rng = np.random.default_rng(RC.SEEDS[name])
    lods = rng.uniform(0.0, 2.0, size=len(rays)).astype(np.float32)
    s = _open(rt64_lib, data)
    lines = []
    try:
        s.draw()
        settings = [0, rt64.RADIANCE_FLAG_UNSHADOWED] + ([rt64.RADIANCE_FLAG_FOG_FROM_CAMERA] if name == "fog_8" else [])
        for flags in settings:
            want = compose(rt64_lib, s.view, data, rays, lods, flags)
            got = rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, want["hits"], lods, flags=flags)
            gb = _bits(got)
            cov = want["coverage"]
            assert np.array_equal(gb[:, 7], _bits(cov)[:, 0]), name                                      # transmittance, bit for bit
            # T7 ends a glass layer's list; W12 does not: none of these scenes has glass, so shaded and COVERED are T7's
            assert np.array_equal(gb[:, 15], _bits(cov)[:, 2]) and np.array_equal(gb[:, 15], want["shaded"].astype(np.uint32))
            assert np.array_equal(gb[:, 11].view(np.int32), want["lit"].astype(np.int32))
            flags_want = np.where(want["valid"], rt64.RADIANCE_VALID, 0) | np.where((_bits(cov)[:, 3] & LR.COVERAGE_COVERED) != 0, rt64.RADIANCE_COVERED, 0) \
                | np.where(want["lit"] >= 0, rt64.RADIANCE_LIT, 0) | np.where(want["fogged"], rt64.RADIANCE_FOGGED, 0)
            assert np.array_equal(gb[:, 3], flags_want.astype(np.uint32)), name
            ok = ~want["near_gate"]
            assert ok.mean() >= 0.995
            ratios = {}
            for field, at in (("radiance", 0), ("surface", 4), ("transparent", 8), ("light", 12)):
                dev = np.abs(got[:, at:at + 3].astype(np.float64) - want[field])
                b = ROUNDINGS * U * want["mag"][field] + want["slack"][field] + 1e-30
                ratios[field] = float((dev / b)[ok].max())
            lines.append("%-10s flags %#05x  rays %3d  lit %3d  fogged %3d  two or more layers %3d  misses %3d  ratio radiance %.3f surface %.3f transparent %.3f light %.3f  lit by a light %3d" %
                         (name, flags, len(rays), int((want["lit"] >= 0).sum()), int(want["fogged"].sum()), int((want["shaded"] >= 2).sum()),
                          int((want["valid"] & (want["shaded"] == 0)).sum()), ratios["radiance"], ratios["surface"], ratios["transparent"], ratios["light"], int((want["direct"].max(axis=1) > 0).sum())))
            print(lines[-1])
            assert (want["shaded"] >= 2).sum() >= 16 and (want["valid"] & (want["shaded"] == 0)).sum() >= 16
            if name == "fog_8":
                assert want["fogged"].sum() >= 16
            if name == "unlit_8":
                assert (want["transparent"].max(axis=1) > 0).sum() >= 16
            assert all(r <= 1.0 for r in ratios.values()), (name, flags, ratios)
            # a ray that misses everything brings back the sky, byte for byte
            miss = want["valid"] & (want["shaded"] == 0)
            assert np.array_equal(gb[miss, 0:3], _bits(want["sky"].astype(np.float32))[miss]) and (got[miss, 7] == 1.0).all()
        if name == "lights_8":          # the light under the floor reaches no sheet: shadowed and unshadowed light differ there
            a = rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, want["hits"], lods, flags=0)
            b = rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, want["hits"], lods, flags=rt64.RADIANCE_FLAG_UNSHADOWED)
            assert (np.abs(a[:, 12:15] - b[:, 12:15]).max(axis=1) > 1e-3).sum() >= 16
    finally:
        s.close()


def test_the_forms_agree_byte_for_byte(rt64_lib, sample_data):
    """5.  Host arrays, device arrays on the device's stream and on a caller stream give the same records; lods = NULL is an array of zeros; lds_cache 0 and 1 agree;
    RT64_TraceViewRayRadiance is the walk and the resolve (W8); maxLayers = m is the resolve over the first m layers of 16; the sky calls' forms agree as well."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K = RC.case(sample_data, "fog_8")
    rays = RC.rays_of(K, 11)
    n = len(rays)
    pixels = np.stack([np.arange(n) % W, (np.arange(n) * 7) % H], axis=1).astype(np.uint32)
    results = []
    for cache in (1, 0):
        s = _open(rt64_lib, data, {"lds_cache": cache})
        hip = ray_rule.Hip()
        try:
            s.draw()
            d_rays, d_lods, d_pix = hip.upload(rays), hip.upload(np.zeros(n, dtype=np.float32)), hip.upload(pixels)
            full, _ = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 16)
            kept = []
            for flags in (0, rt64.RADIANCE_FLAG_UNSHADOWED, rt64.RADIANCE_FLAG_FOG_FROM_CAMERA | CULL):
                for m in (16, 3):
                    hits, layers, rad = rt64.trace_view_ray_radiance(rt64_lib, s.view, rays, m, flags=flags)
                    h2, l2 = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, m, flags=flags & CULL)
                    r2 = rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, h2, flags=flags)
                    for x, y in ((hits, h2), (layers, l2), (rad, r2)):
                        assert np.array_equal(_bits(x), _bits(y))                               # W8
                    only = rt64.trace_view_ray_radiance(rt64_lib, s.view, rays, m, flags=flags, hits=False, layers=False)
                    assert np.array_equal(_bits(only), _bits(rad))
                    if not flags & CULL:
                        assert np.array_equal(_bits(rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, full[:m], flags=flags)), _bits(rad))      # the first m of 16
                    assert ((_bits(rad)[:, 15] >= 2).sum() > 60) and ((_bits(rad)[:, 3] & rt64.RADIANCE_FOGGED) != 0).sum() > 30
                    kept.append(rad)
                    for st, l in ((None, None), (hip.stream(), d_lods)):
                        d_hits, d_rad = hip.upload(h2), hip.alloc(rad.nbytes)
                        assert rt64_lib.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, l, m, d_rad, n, flags, st) == 1, rt64_lib.last_error()
                        if st:
                            assert hip.h.hipStreamSynchronize(st) == 0
                        assert np.array_equal(_bits(hip.download(d_rad, rad)), _bits(rad))
            sky, psky, rows = rt64.sky_view_rays(rt64_lib, s.view, rays), rt64.sky_view_pixels(rt64_lib, s.view, pixels), rt64.sky_view_pixels(rt64_lib, s.view, count=n)
            listed = np.stack([np.arange(n) % W, np.arange(n) // W], axis=1).astype(np.uint32)
            assert np.array_equal(_bits(rt64.sky_view_pixels(rt64_lib, s.view, listed)), _bits(rows))          # pixels = NULL counts them row by row
            kept += [sky, psky]
            for st in (None, hip.stream()):
                d_a, d_b = hip.alloc(sky.nbytes), hip.alloc(psky.nbytes)
                assert rt64_lib.SkyViewRaysDevice(s.view, d_rays, d_a, n, st) == 1, rt64_lib.last_error()
                assert rt64_lib.SkyViewPixelsDevice(s.view, d_pix, d_b, n, st) == 1, rt64_lib.last_error()
                if st:
                    assert hip.h.hipStreamSynchronize(st) == 0
                assert np.array_equal(_bits(hip.download(d_a, sky)), _bits(sky)) and np.array_equal(_bits(hip.download(d_b, psky)), _bits(psky))
            results.append(kept)
        finally:
            hip.close()
            s.close()
    for x, y in zip(*results):
        assert np.array_equal(_bits(x), _bits(y))                                               # lds_cache 1 against 0


def test_sizes_grid_stride_and_the_ends_of_the_arrays(rt64_lib, sample_data):
    """6.  Counts 1, 63, 64, 65, 255, 256, 257 and RT_GRID_BLOCKS x RT_BLOCK + 1 at maxLayers = 1, where the stride loop runs twice: each record equals the ray's own
    whatever its place, every slot is written and the guard words before and after each output array are untouched, on the device forms and (the small counts) the
    host forms, for the radiance records and both kinds of sky record."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K = RC.case(sample_data, "stack_8")
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = RC.rays_of(K, 29)
        big, m = 2048 * 256 + 1, 1
        reps = -(-big // len(rays))
        rng = np.random.default_rng(5)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(reps - 1)])[:big]
        many = np.ascontiguousarray(rays[order])
        pixels = np.stack([np.arange(len(rays)) % W, np.arange(len(rays)) % H], axis=1).astype(np.uint32)
        many_pixels = np.ascontiguousarray(pixels[order])
        fh, _, fr = rt64.trace_view_ray_radiance(rt64_lib, s.view, rays, m)
        fs, fp = rt64.sky_view_rays(rt64_lib, s.view, rays), rt64.sky_view_pixels(rt64_lib, s.view, pixels)
        d_rays, d_pixels = hip.upload(many), hip.upload(many_pixels)
        d_hits = hip.upload(np.ascontiguousarray(fh[:, order]))
        pad = 8          # guard records in front of and behind every output array
        for count in (1, 63, 64, 65, 255, 256, 257, big):
            want = [_bits(fr)[order[:count]], _bits(fs)[order[:count]], _bits(fp)[order[:count]]]
            shapes = [(count + 2 * pad, 16), (count + 2 * pad, 8), (count + 2 * pad, 8)]
            bufs = [hip.upload(np.full(sh, GUARD, dtype=np.uint32)) for sh in shapes]
            first = [b + pad * sh[1] * 4 for b, sh in zip(bufs, shapes)]
            assert rt64_lib.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, None, m, first[0], count, 0, None) == 1, rt64_lib.last_error()
            assert rt64_lib.SkyViewRaysDevice(s.view, d_rays, first[1], count, None) == 1, rt64_lib.last_error()
            assert rt64_lib.SkyViewPixelsDevice(s.view, d_pixels, first[2], count, None) == 1, rt64_lib.last_error()
            for b, sh, w in zip(bufs, shapes, want):
                out = hip.download(b, np.empty(sh, dtype=np.uint32))
                assert (out[:pad] == GUARD).all() and np.array_equal(out[pad:pad + count], w) and (out[pad + count:] == GUARD).all(), (count, sh)
            if count <= 257:
                host = [np.full(sh, GUARD, dtype=np.uint32) for sh in shapes]
                at = [h[pad:].ctypes.data for h in host]
                hits_in = np.ascontiguousarray(fh[:, order[:count]])
                assert rt64_lib.ComposeViewRayRadiance(s.view, many.ctypes.data, hits_in.ctypes.data, None, m, at[0], count, 0) == 1, rt64_lib.last_error()
                assert rt64_lib.SkyViewRays(s.view, many.ctypes.data, at[1], count) == 1 and rt64_lib.SkyViewPixels(s.view, many_pixels.ctypes.data, at[2], count) == 1
                for out, w in zip(host, want):
                    assert (out[:pad] == GUARD).all() and np.array_equal(out[pad:pad + count], w) and (out[pad + count:] == GUARD).all(), count
                traced = np.full(shapes[0], GUARD, dtype=np.uint32)
                assert rt64_lib.TraceViewRayRadiance(s.view, many.ctypes.data, None, m, None, None, traced[pad:].ctypes.data, count, 0) == 1, rt64_lib.last_error()
                assert (traced[:pad] == GUARD).all() and np.array_equal(traced[pad:pad + count], want[0]) and (traced[pad + count:] == GUARD).all()
            for b in bufs:
                assert hip.h.hipFree(b) == 0
                hip.ptrs.remove(b)
    finally:
        hip.close()
        s.close()


@pytest.mark.parametrize("m, count", [(16, 16384 + 65), (3, 87381 + 1)])
def test_host_arrays_that_cross_a_chunk_agree_with_the_device_form(rt64_lib, sample_data, m, count):
    """6b.  The host forms stage 2^18 / maxLayers rays per round trip.  One ray more than a chunk (65 more at 16 layers): RT64_ComposeViewRayRadiance fed with the device
    walk's hits (the layer-major gather on the way up) and RT64_TraceViewRayRadiance equal the device form, which does not chunk, bit for bit, and the spare records
    behind each host array keep their guard words."""
    data, K = RC.case(sample_data, "fog_8")
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = RC.rays_of(K, 29)
        rng = np.random.default_rng(7)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(-(-count // len(rays)) - 1)])[:count]
        many = np.ascontiguousarray(rays[order])
        d_rays = hip.upload(many)
        d_hits, d_lay, d_rad = hip.alloc(m * count * 32), hip.alloc(count * 16), hip.alloc(count * 64)
        assert rt64_lib.TraceViewRayLayersDevice(s.view, d_rays, None, m, d_hits, d_lay, count, 0, None) == 1, rt64_lib.last_error()
        assert rt64_lib.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, None, m, d_rad, count, 0, None) == 1, rt64_lib.last_error()
        hits = hip.download(d_hits, np.empty((m * count, 8), dtype=np.uint32))
        lay = hip.download(d_lay, np.empty((count, 4), dtype=np.uint32))
        want = hip.download(d_rad, np.empty((count, 16), dtype=np.uint32))
        assert (want[:, 15] >= 2).sum() >= 32 and len(np.unique(want[:, 0])) > 32
        out = np.full((count + 7, 16), GUARD, dtype=np.uint32)
        assert rt64_lib.ComposeViewRayRadiance(s.view, many.ctypes.data, hits.ctypes.data, None, m, out.ctypes.data, count, 0) == 1, rt64_lib.last_error()
        assert np.array_equal(out[:count], want) and (out[count:] == GUARD).all()
        out = np.full((count + 7, 16), GUARD, dtype=np.uint32)
        h2, l2 = np.full((m * count + 7, 8), GUARD, dtype=np.uint32), np.full((count + 7, 4), GUARD, dtype=np.uint32)
        assert rt64_lib.TraceViewRayRadiance(s.view, many.ctypes.data, None, m, h2.ctypes.data, l2.ctypes.data, out.ctypes.data, count, 0) == 1, rt64_lib.last_error()
        assert np.array_equal(out[:count], want) and (out[count:] == GUARD).all()
        assert np.array_equal(h2[:m * count], hits) and (h2[m * count:] == GUARD).all() and np.array_equal(l2[:count], lay) and (l2[count:] == GUARD).all()
    finally:
        hip.close()
        s.close()


def test_bad_records_and_invalid_rays(rt64_lib, sample_data):
    """7.  W3: an out-of-range instance or primitive at layer 0 gives BAD_HIT and the sky alone; placed behind complete coverage it is never read; in front of it, it
    ends the list with BAD_HIT and what was gathered before it stays; a Q6-invalid ray gives the zero record with flags 0, transmittance 1 and litLayer -1, whatever its hits say."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K = RC.case(sample_data, "stack_3")
    rays = RC.rays_of(K, RC.SEEDS["stack_3"])
    s = _open(rt64_lib, data)
    try:
        s.draw()
        hits, layers = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 8)
        count = layers[:, 0].astype(np.int64)
        good = rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, hits)
        sky = rt64.sky_view_rays(rt64_lib, s.view, rays)
        gf = _bits(good)[:, 3]
        valid, covered = (gf & rt64.RADIANCE_VALID) != 0, (gf & rt64.RADIANCE_COVERED) != 0
        bad = hits.copy(); bb = _bits(bad)
        for k in range(len(rays)):
            bb[count[k], k, 3] = 1000 + k; bb[count[k], k, 4] = 0
        got = rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, bad)
        assert covered.sum() >= 32 and (valid & ~covered).sum() >= 32
        assert np.array_equal(_bits(got)[covered], _bits(good)[covered])                          # behind complete coverage: not read
        open_ = valid & ~covered
        assert np.array_equal(_bits(got)[open_, 3], gf[open_] | rt64.RADIANCE_BAD_HIT)
        keep = [c for c in range(16) if c != 3]
        assert np.array_equal(_bits(got)[open_][:, keep], _bits(good)[open_][:, keep])            # what was gathered before it stays
        for column, value in ((3, 0x7FFFFFF0), (4, 0x00FFFFFF)):                                 # layer 0: an instance, then a primitive, out of range
            bad = hits.copy(); bb = _bits(bad)
            bb[0, :, column] = value
            got = rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, bad)
            first = valid & (count > 0)
            assert first.sum() >= 100
            assert (_bits(got)[first, 3] == (rt64.RADIANCE_VALID | rt64.RADIANCE_BAD_HIT)).all() and (got[first, 7] == 1.0).all()
            assert np.array_equal(_bits(got)[first, 0:3], _bits(sky)[first, 0:3]) and (_bits(got)[first, 11].view(np.int32) == -1).all() and not _bits(got)[first, 15].any()
        invalid = ~valid
        assert invalid.sum() >= 8
        bad = hits.copy(); _bits(bad)[:, invalid, 3] = 0; _bits(bad)[:, invalid, 4] = 0          # real records behind an invalid ray: not read
        got = rt64.resolve_view_ray_radiance(rt64_lib, s.view, rays, bad)
        zero = np.zeros(16, dtype=np.uint32); zero[7] = _bits(np.float32(1.0).reshape(1))[0]; zero[11] = 0xFFFFFFFF
        assert (_bits(got)[invalid] == zero[None]).all()
        assert not _bits(sky)[invalid].any()                                                      # W1: zeros, flags 0
        assert np.array_equal(_bits(got)[valid], _bits(good)[valid])
    finally:
        s.close()


def test_the_sky_records(rt64_lib, sample_data):
    """W1 / W2 on their own: the flags say what the frame had (a sky texture, a raster background), the record of a scene without a sky texture has alpha 0, the uv of a
    direction lies in [0, 1], a Q6-invalid ray gives zeros, and a pixel outside the frame extrapolates: its uv continues the frame's, linearly."""
    from sm64rt_legacy_renderer_amd import rt64
    rays = RC.rays_of(3, 5)
    valid = np.array([ray_rule.ray_is_valid(r) for r in rays])
    pixels = np.array([[0, 0], [W - 1, H - 1], [W, H], [3 * W, 7], [5, 2 * H]], dtype=np.uint32)
    seen = {}
    for name, flags in (("stack_3", rt64.SKY_VALID), ("nosky_3", rt64.SKY_VALID | rt64.SKY_NO_TEXTURE)):
        data, K = RC.case(sample_data, name)
        s = _open(rt64_lib, data)
        try:
            s.draw()
            sky, psky = rt64.sky_view_rays(rt64_lib, s.view, rays), rt64.sky_view_pixels(rt64_lib, s.view, pixels)
        finally:
            s.close()
        seen[name] = (sky, psky)
        background = _bits(sky)[valid, 6] & rt64.SKY_BACKGROUND
        assert (background == background[0]).all() and (_bits(psky)[:, 6] & rt64.SKY_BACKGROUND == background[0]).all()          # one frame, one answer
        assert (_bits(sky)[valid, 6] & (0xFFFFFFFF ^ rt64.SKY_BACKGROUND) == flags).all() and not _bits(sky)[:, 7].any()
        assert (_bits(psky)[:, 6] & (0xFFFFFFFF ^ rt64.SKY_BACKGROUND) == flags).all()
        assert valid.sum() >= 100 and (~valid).sum() >= 8 and not _bits(sky)[~valid].any()
        assert ((sky[valid, 4:6] >= 0.0) & (sky[valid, 4:6] <= 1.0)).all()
        assert ((sky[valid, 3] >= 0.0) & (sky[valid, 3] <= 1.0)).all()
        if name == "nosky_3":
            assert (sky[:, 3] == 0.0).all() and (psky[:, 3] == 0.0).all()
        else:
            assert len(np.unique(sky[valid, 0])) > 16 and sky[valid, :3].max() > 0.0          # the sample's clouds vary
        du = float(psky[1, 4]) - float(psky[0, 4])
        assert du != 0.0 and abs((float(psky[2, 4]) - float(psky[0, 4])) - du * W / (W - 1)) <= 16 * U * abs(float(psky[2, 4])) + 1e-7
    assert np.array_equal(_bits(seen["stack_3"][0])[:, 4:6], _bits(seen["nosky_3"][0])[:, 4:6])          # uv is reported with or without a texture


def _sky_variant(sample_data, name):
    """The small sample scene under another sky: a yaw offset; a multiplier and an HSL modifier on all three components; a generated texture whose alpha runs from 0 to 1 (64 x 32,
    so a frame with reflections would also make its tiled copy), which lets the raster background through."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    d = MC.small_sample(sample_data)          # the sphere on the floor: the upper half of the picture is sky
    d.desc = copy.copy(d.desc)
    d.textures = list(d.textures)
    d.textures[d.sky] = sample_data.textures[sample_data.sky]          # the sample's clouds (small_sample's sky is one flat colour)
    if name == "yaw":
        d.desc.skyYawOffset = 0.7
    elif name == "hsl":
        d.desc.skyDiffuseMultiplier = rt64.VECTOR3(0.8, 1.1, 0.9); d.desc.skyHSLModifier = rt64.VECTOR3(0.1, -0.2, 0.15)
    else:
        y, x = np.mgrid[0:32, 0:64]
        texels = np.stack([(x * 4) % 256, (y * 8) % 256, (x * 3 + y * 5) % 256, (x * 4 + y) % 256], axis=-1).astype(np.uint8)
        d.textures.append(sample_scene.TextureData("sky-alpha", rt64.TEXTURE_FORMAT_RGBA8, texels, 64, 32))
        d.sky = len(d.textures) - 1
    return d


@pytest.mark.parametrize("name", ["yaw", "hsl", "translucent"])
def test_the_sky_of_a_pixel_is_what_the_frame_shows_there(rt64_lib, sample_data, name):
    """3.  Against the frame: at the pixels whose camera ray has an empty list the primary resolve stores the background term alone, bgColor x 1, in RT64_IMAGE_DIFFUSE
    (RGBA8).  RT64_SkyViewPixels runs the same functions on the same screenUV, so its colour, clamped to [0, 1], must lie within half a UNORM8 step (plus four float32
    roundings for the conversion) of the stored one -- under a yaw offset, under a multiplier with an HSL modifier, and with a translucent sky over the raster
    background.  The pixel form with pixels = NULL, with the pixels listed, and the ray form along the camera ray's direction are compared as well: the envmap uv of
    a direction is not the plane's uv of a pixel, so the ray form differs from the pixel form wherever the sky varies (W1 against W2)."""
    from sm64rt_legacy_renderer_amd import rt64
    data = _sky_variant(sample_data, name)
    s = _open(rt64_lib, data, {"lean_frames": 0})
    try:
        s.draw()
        diffuse = s.readback(rt64.IMAGE_DIFFUSE).reshape(-1, 4)
        rays = rt64.camera_rays(rt64_lib, s.view, count=W * H, differentials=False)
        _, layers = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 1, flags=CULL)
        psky = rt64.sky_view_pixels(rt64_lib, s.view, count=W * H)
        rsky = rt64.sky_view_rays(rt64_lib, s.view, rays)
    finally:
        s.close()
    empty = layers[:, 0] == 0
    assert empty.sum() >= 500
    want = diffuse[empty, :3].astype(np.float64)
    got = np.clip(psky[empty, :3].astype(np.float64), 0.0, 1.0)
    dev = np.abs(got - want)
    print("sky %-12s empty pixels %4d  largest |sky_view_pixels - DIFFUSE| %.5f of a UNORM8 step  alpha %.3f .. %.3f  background flag %d" %
          (name, int(empty.sum()), float(dev.max() * 255.0), float(psky[empty, 3].min()), float(psky[empty, 3].max()), int(_bits(psky)[0, 6] & rt64.SKY_BACKGROUND) != 0))
    assert (dev <= 0.5 / 255.0 + 4 * U).all(), float(dev.max() * 255.0)
    assert len(np.unique(want[:, 0])) > 8                                                      # a sky that varies over those pixels
    if name == "translucent":
        assert psky[empty, 3].min() < 0.5 < psky[empty, 3].max()
    assert (np.abs(rsky[empty, :3] - psky[empty, :3]).max(axis=1) > 1.0 / 255.0).sum() >= 100          # W1 is not W2


def test_radiance_against_the_frames_mirror_pass(rt64_lib, sample_data):
    """4.  Against the frame: tests/mirror_cases.py's `sky` scene -- mirror_cases._base with a mirror floor, a translucent sphere, two translucent panes one behind the
    other, none of which mirrors, one light, a sky -- with the floor's reflectionShineFactor 0, diSamples = 0, lean_frames = 0.  Session 0 (max_reflections = 0) stores
    what the pass reads: position, view direction, normal, instance id and REFLECTION = (0, 0, 0, reflA).  Session 1 (max_reflections = 1) stores REFLECTION after the
    pass.  The query's ray is built on the host in float32 from the stored values, { position, 0.1, reflect(view, normal), 100000 }, and asked UNSHADOWED with the
    frame's back-face culling.  Where no mirror is seen in the mirror, and with no shine, the pass adds rgb x reflA, so radiance x reflA must lie within
    mirror_rule.reflection_pass's own per-pixel bound of the rule's value at every pixel it takes and decides -- the rule is the reference, the query gets no margin
    of its own -- and so must the stored image.  RT64_SkyViewRays along the same rays must be the sky term that rule uses."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    import mirror_cases
    import mirror_rule
    case = mirror_cases.make_case(sample_data, "sky")
    data = case["data_at"](0)
    floor = next(i for i in data.instances if i.name == "floor")
    floor.material.reflectionShineFactor = 0.0
    assert len(data.lights) == 1 and case["view"]["di_samples"] == 0
    stored = {}
    for k in (0, 1):
        s = sample_scene.Rt64Scene(rt64_lib, data, W, H, hip_device=0)
        try:
            s.set_view_description(**case["view"])
            assert s.option("max_reflections", k) and s.option("lean_frames", 0)
            s.draw()
            stored[k] = {key: s.readback(getattr(rt64, "IMAGE_" + name)).copy() for key, name in mirror_cases.GPU_IMAGES.items()}
            if k == 1:
                a = stored[0]
                takes = (a["id"] >= 0) & (a["reflection"][..., 3] > mirror_rule.EPSILON)
                pos = a["position"][takes][:, :3].astype(np.float32); v = a["view"][takes][:, :3].astype(np.float32); nr = a["normal"][takes][:, :3].astype(np.float32)
                dot = ((nr[:, 0] * v[:, 0] + nr[:, 1] * v[:, 1]) + nr[:, 2] * v[:, 2]).astype(np.float32)
                d = (v - nr * (F32(2.0) * dot)[:, None]).astype(np.float32)                      # device_math.h: reflect3
                rays = np.zeros((len(pos), 8), dtype=np.float32)
                rays[:, 0:3] = pos; rays[:, 3] = F32(0.1); rays[:, 4:7] = d; rays[:, 7] = F32(100000.0)
                got = rt64.trace_view_ray_radiance(rt64_lib, s.view, rays, 16, flags=rt64.RADIANCE_FLAG_UNSHADOWED | CULL, hits=False, layers=False)
                sky = rt64.sky_view_rays(rt64_lib, s.view, rays)
        finally:
            s.close()
    for key in mirror_cases.STATE:          # the same G-buffer in both sessions where no pass works (where one does, session 1's readback folds the continuation state in)
        assert np.array_equal(np.asarray(stored[0][key])[~takes], np.asarray(stored[1][key])[~takes]), key
    scene = mirror_cases.rule_scene(data, case["view"], 0)
    rule = mirror_rule.reflection_pass(scene, a["position"], a["view"], a["normal"], a["id"], a["reflection"])
    assert np.array_equal(rule["takes"], takes)
    decided = (rule["decided"] & takes)[takes]
    # The floor itself is seen in the floor (a ninth of the pixels, near its far edge and behind the panes): there the pass adds a Fresnel share to the next pass's alpha and
    # weighs this one by k = reflA x saturate(1 - that share) instead of reflA -- W12's "k weight", which belongs to the surface the ray left.  The identity is asked
    # where the rule says no mirror was seen in the mirror; the other pixels are counted.
    plain = rule["info"]["fresnel_alpha"][takes] == 0.0
    ok = decided & plain
    refl_a = a["reflection"][takes][:, 3].astype(np.float64)
    value, bound = rule["value"][takes][:, :3], rule["bound"][takes][:, :3]
    after = stored[1]["reflection"][takes][:, :3].astype(np.float64)
    mine = got[:, 0:3].astype(np.float64) * refl_a[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        r_query = np.where(mine == value, 0.0, np.abs(mine - value) / bound).max(axis=1)
        r_frame = np.where(after == value, 0.0, np.abs(after - value) / bound).max(axis=1)
    layers = _bits(got)[:, 15]
    sees_object, sees_sky = ok & (layers > 0), ok & (got[:, 7] > 0.0)
    print("mirror pass: pixels taken %4d  a mirror in the mirror %4d  decided %4d  see an object %4d  see the sky %4d  two or more layers %4d  largest |radiance x reflA - rule| / bound %.4f  "
          "largest |REFLECTION - rule| / bound %.4f  largest |radiance x reflA - REFLECTION| %.3e" %
          (int(takes.sum()), int((~plain).sum()), int(ok.sum()), int(sees_object.sum()), int(sees_sky.sum()), int((ok & (layers >= 2)).sum()), float(r_query[ok].max()), float(r_frame[ok].max()),
           float(np.abs(mine - after)[ok].max())))
    assert ok.sum() >= 200 and sees_object.sum() >= 50 and sees_sky.sum() >= 50 and (ok & (layers >= 2)).sum() >= 16
    assert (~decided).sum() <= int(mirror_cases.UNDECIDED_CAP * takes.sum()) and (~plain).sum() < 0.5 * takes.sum()
    assert (r_frame[decided] < 1.0).all()                                                               # the frame itself, as tests/test_gpu_mirror_rule.py holds it
    assert (r_query[ok] < 1.0).all(), (float(r_query[ok].max()), np.nonzero(ok & ~(r_query < 1.0))[0][:8].tolist())
    # what the rule says of the rays: a surface where the query has a lit layer, the same instance
    assert np.array_equal((rule["has_hit"][takes])[ok], (_bits(got)[:, 11].view(np.int32) >= 0)[ok])
    # the sky term: one constant colour (the texels are all equal), times the multiplier
    term = np.array([c.v for c in scene["sky"]], dtype=np.float64).reshape(3); term_e = np.array([np.max(c.e) for c in scene["sky"]], dtype=np.float64).reshape(3)
    assert (np.abs(sky[:, 0:3].astype(np.float64) - term[None]) <= term_e[None] + U * term[None]).all() and (sky[:, 3] == 1.0).all()
    miss = layers == 0
    assert miss.sum() >= 16 and np.array_equal(_bits(got)[miss, 0:3], _bits(sky)[miss, 0:3])


def test_refusals(rt64_lib, sample_data):
    """8.  W10, one by one: every refusal returns 0 with a message that names the function; count = 0 succeeds and touches nothing; RT64_SetMesh refuses the radiance
    calls, a destroyed surface texture refuses them too, a destroyed sky texture refuses every call of the header, each until the next frame."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    data = MC.small_sample(sample_data)
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    R_ = rt64_lib
    try:
        rays = ray_rule.random_rays(data, 31, 600, floor_instance=3)
        n, m = len(rays), 2
        hits = np.full((m, n, 8), GUARD, dtype=np.uint32); lay = np.full((n, 4), GUARD, dtype=np.uint32)
        rad = np.full((n, 16), GUARD, dtype=np.uint32); sky = np.full((n, 8), GUARD, dtype=np.uint32)
        pixels = np.zeros((n, 2), dtype=np.uint32)
        d_rays, d_hits, d_rad, d_sky, d_pix = hip.upload(rays), hip.upload(hits), hip.alloc(rad.nbytes), hip.alloc(sky.nbytes), hip.upload(pixels)
        d_lods = hip.upload(np.zeros(n, dtype=np.float32))
        rp, hp, lp, ap, sp, pp = rays.ctypes.data, hits.ctypes.data, lay.ctypes.data, rad.ctypes.data, sky.ctypes.data, pixels.ctypes.data
        C_, CD, T = "RT64_ComposeViewRayRadiance", "RT64_ComposeViewRayRadianceDevice", "RT64_TraceViewRayRadiance"
        SR, SRD, SP, SPD = "RT64_SkyViewRays", "RT64_SkyViewRaysDevice", "RT64_SkyViewPixels", "RT64_SkyViewPixelsDevice"

        def refused(word, fn, call):
            ok = call()
            assert ok == 0 and fn + ":" in R_.last_error() and word in R_.last_error(), (ok, R_.last_error())

        def radiance_refused(word):
            refused(word, C_, lambda: R_.ComposeViewRayRadiance(s.view, rp, hp, None, m, ap, n, 0))
            refused(word, CD, lambda: R_.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, None, m, d_rad, 4, 0, None))
            refused(word, T, lambda: R_.TraceViewRayRadiance(s.view, rp, None, m, hp, lp, ap, n, 0))

        def sky_refused(word):
            refused(word, SR, lambda: R_.SkyViewRays(s.view, rp, sp, n))
            refused(word, SRD, lambda: R_.SkyViewRaysDevice(s.view, d_rays, d_sky, 4, None))
            refused(word, SP, lambda: R_.SkyViewPixels(s.view, pp, sp, n))
            refused(word, SPD, lambda: R_.SkyViewPixelsDevice(s.view, d_pix, d_sky, 4, None))
        radiance_refused("draw"); sky_refused("draw")                                     # before the first frame
        s.draw()
        assert R_.ComposeViewRayRadiance(s.view, rp, hp, None, m, ap, 0, 0) == 1 and R_.TraceViewRayRadiance(s.view, rp, None, m, hp, lp, ap, 0, 0) == 1
        assert R_.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, None, m, d_rad, 0, 0, None) == 1
        assert R_.SkyViewRays(s.view, rp, sp, 0) == 1 and R_.SkyViewPixels(s.view, pp, sp, 0) == 1
        assert R_.SkyViewRaysDevice(s.view, d_rays, d_sky, 0, None) == 1 and R_.SkyViewPixelsDevice(s.view, d_pix, d_sky, 0, None) == 1
        for bad in (0, 17, 0xFFFFFFFF):
            refused("maxLayers", C_, lambda: R_.ComposeViewRayRadiance(s.view, rp, hp, None, bad, ap, 4, 0))
            refused("maxLayers", CD, lambda: R_.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, None, bad, d_rad, 4, 0, None))
            refused("maxLayers", T, lambda: R_.TraceViewRayRadiance(s.view, rp, None, bad, hp, lp, ap, 4, 0))
        for flags in (0x2, 0x4, 0x400, 0x80000000):
            refused("unknown flags", C_, lambda: R_.ComposeViewRayRadiance(s.view, rp, hp, None, m, ap, 4, flags))
            refused("unknown flags", CD, lambda: R_.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, None, m, d_rad, 4, flags, None))
            refused("unknown flags", T, lambda: R_.TraceViewRayRadiance(s.view, rp, None, m, hp, lp, ap, 4, flags))
        refused("NULL", C_, lambda: R_.ComposeViewRayRadiance(s.view, None, hp, None, m, ap, 4, 0))
        refused("NULL", C_, lambda: R_.ComposeViewRayRadiance(s.view, rp, None, None, m, ap, 4, 0))
        refused("NULL", C_, lambda: R_.ComposeViewRayRadiance(s.view, rp, hp, None, m, None, 4, 0))
        refused("NULL view", C_, lambda: R_.ComposeViewRayRadiance(None, rp, hp, None, m, ap, 4, 0))
        refused("NULL", CD, lambda: R_.ComposeViewRayRadianceDevice(s.view, d_rays, None, None, m, d_rad, 4, 0, None))
        refused("NULL", T, lambda: R_.TraceViewRayRadiance(s.view, None, None, m, hp, lp, ap, 4, 0))
        refused("NULL", T, lambda: R_.TraceViewRayRadiance(s.view, rp, None, m, hp, lp, None, 4, 0))
        refused("NULL", SR, lambda: R_.SkyViewRays(s.view, None, sp, 4))
        refused("NULL", SR, lambda: R_.SkyViewRays(s.view, rp, None, 4))
        refused("NULL", SP, lambda: R_.SkyViewPixels(s.view, pp, None, 4))
        refused("NULL view", SPD, lambda: R_.SkyViewPixelsDevice(None, d_pix, d_sky, 4, None))
        refused("more records", SP, lambda: R_.SkyViewPixels(s.view, None, sp, W * H + 1))
        for a, l, b, c in ((d_rays + 4, None, d_hits, d_rad), (d_rays, None, d_hits + 8, d_rad), (d_rays, None, d_hits, d_rad + 4), (d_rays, d_lods + 2, d_hits, d_rad)):
            refused("aligned", CD, lambda: R_.ComposeViewRayRadianceDevice(s.view, a, b, l, m, c, 4, 0, None))
        refused("aligned", SRD, lambda: R_.SkyViewRaysDevice(s.view, d_rays + 8, d_sky, 4, None))
        refused("aligned", SRD, lambda: R_.SkyViewRaysDevice(s.view, d_rays, d_sky + 4, 4, None))
        refused("aligned", SPD, lambda: R_.SkyViewPixelsDevice(s.view, d_pix + 4, d_sky, 4, None))
        refused("aligned", SPD, lambda: R_.SkyViewPixelsDevice(s.view, d_pix, d_sky + 8, 4, None))
        assert (hits == GUARD).all() and (lay == GUARD).all() and (rad == GUARD).all() and (sky == GUARD).all()
        real_hits, _ = rt64.trace_view_ray_layers(R_, s.view, rays, m)
        d_real = hip.upload(real_hits)
        assert R_.ComposeViewRayRadianceDevice(s.view, d_rays, d_real, d_lods + 4, m, d_rad, 4, 0, None) == 1          # lods need 4-byte alignment only
        assert R_.SkyViewPixelsDevice(s.view, d_pix + 8, d_sky, 4, None) == 1                                            # and pixels 8
        want = rt64.trace_view_ray_radiance(R_, s.view, rays, m)
        want_sky = rt64.sky_view_rays(R_, s.view, rays)
        # RT64_SetMesh on a mesh the frame traced: the radiance calls are refused until the next frame; the sky calls read no mesh
        msh = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], msh.vertices, msh.indices)
        radiance_refused("RT64_SetMesh")
        assert np.array_equal(_bits(rt64.sky_view_rays(R_, s.view, rays)), _bits(want_sky))
        s.draw()
        # RT64_DestroyTexture of a surface texture the frame's table holds (a copy of the floor's diffuse map on an extra instance, which goes first)
        t = data.textures[4]
        td = rt64.TEXTURE_DESC(); buf, pitch = t.upload_buffer()
        td.bytes = buf.ctypes.data; td.byteCount = buf.nbytes; td.format = t.format; td.width, td.height, td.rowPitch = t.width, t.height, pitch
        th = R_.CreateTexture(s.device, td)
        assert th, R_.last_error()
        s.textures.append(th)
        ih = R_.CreateInstance(s.scene); s.instances.append(ih)
        far = copy.copy(data.instances[1])
        tr = np.array(far.transform, dtype=np.float32).copy(); tr[3, 0] -= np.float32(3.0)
        s.set_instance(len(s.instances) - 1, sample_scene.InstanceData("extra", far.mesh, tr, tr, len(s.textures) - 1, None, None, far.material))
        s.draw()
        assert rt64.trace_view_ray_radiance(R_, s.view, rays, m) is not None
        R_.DestroyInstance(ih); s.instances.pop()
        R_.DestroyTexture(th); s.textures.pop()
        radiance_refused("texture")
        assert np.array_equal(_bits(rt64.sky_view_rays(R_, s.view, rays)), _bits(want_sky))          # the sky calls read no surface texture
        s.draw()
        got = rt64.trace_view_ray_radiance(R_, s.view, rays, m)
        for x, y in zip(got, want):
            assert np.array_equal(_bits(x), _bits(y))
        # RT64_DestroyTexture of the sky texture: a copy of it becomes the view's sky plane for one frame, then goes
        t = data.textures[data.sky]
        td = rt64.TEXTURE_DESC(); buf, pitch = t.upload_buffer()
        td.bytes = buf.ctypes.data; td.byteCount = buf.nbytes; td.format = t.format; td.width, td.height, td.rowPitch = t.width, t.height, pitch
        th = R_.CreateTexture(s.device, td)
        assert th, R_.last_error()
        R_.SetViewSkyPlane(s.view, th)
        s.draw()
        assert np.array_equal(_bits(rt64.sky_view_rays(R_, s.view, rays)), _bits(want_sky))          # the same texels
        R_.SetViewSkyPlane(s.view, s.textures[data.sky])
        R_.DestroyTexture(th)
        radiance_refused("sky texture"); sky_refused("sky texture")
        s.draw()
        got = rt64.trace_view_ray_radiance(R_, s.view, rays, m)
        for x, y in zip(got, want):
            assert np.array_equal(_bits(x), _bits(y))
        assert np.array_equal(_bits(rt64.sky_view_rays(R_, s.view, rays)), _bits(want_sky))
    finally:
        hip.close()
        s.close()


def test_a_resolve_on_a_caller_stream_outlives_its_texture(rt64_lib, sample_data):
    """8b.  K9's texture lifetime: enqueued on a caller's stream, followed at once by RT64_DestroyTexture of a texture the resolve reads (the edge sheet's) and by a new
    frame: the records are the bytes of the synchronous call made before it."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K = RC.case(sample_data, "edge_8")
    rays = RC.rays_of(K, 21)
    s = _open(rt64_lib, data, {"sync_present": 0})
    hip = ray_rule.Hip()
    try:
        edge = data.edge_instance
        t = data.textures[data.instances[edge].diffuse]
        td = rt64.TEXTURE_DESC(); buf, pitch = t.upload_buffer()
        td.bytes = buf.ctypes.data; td.byteCount = buf.nbytes; td.format = t.format; td.width, td.height, td.rowPitch = t.width, t.height, pitch
        th = rt64_lib.CreateTexture(s.device, td)
        s.textures.append(th)
        sheet = copy.copy(data.instances[edge]); sheet.diffuse = len(s.textures) - 1
        s.set_instance(edge, sheet)
        s.draw()
        hits, _, first = rt64.trace_view_ray_radiance(rt64_lib, s.view, rays, 4)
        sky = rt64.sky_view_rays(rt64_lib, s.view, rays)
        reps = 64
        many = np.ascontiguousarray(np.tile(rays, (reps, 1)))
        many_hits = np.ascontiguousarray(np.tile(hits, (1, reps, 1)))
        like, like_sky = np.empty((len(many), 16), dtype=np.float32), np.empty((len(many), 8), dtype=np.float32)
        d_rays, d_hits, d_rad, d_sky = hip.upload(many), hip.upload(many_hits), hip.alloc(like.nbytes), hip.alloc(like_sky.nbytes)
        st = hip.stream()
        assert rt64_lib.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, None, 4, d_rad, len(many), 0, st) == 1, rt64_lib.last_error()
        assert rt64_lib.SkyViewRaysDevice(s.view, d_rays, d_sky, len(many), st) == 1, rt64_lib.last_error()
        s.set_instance(edge, data.instances[edge])
        rt64_lib.DestroyTexture(th); s.textures.pop()
        s.draw()
        got = _bits(hip.download(d_rad, like)).reshape(reps, len(rays), 16)
        assert (got == _bits(first)[None]).all()
        assert (_bits(hip.download(d_sky, like_sky)).reshape(reps, len(rays), 8) == _bits(sky)[None]).all()
    finally:
        hip.close()
        s.close()


@pytest.mark.parametrize("streams", [1, 3])
def test_radiance_queries_between_frames_leave_the_frames_alone(rt64_lib, sample_data, streams, monkeypatch):
    """8c.  A GI + denoiser sequence with radiance and sky queries between its frames -- host arrays, and device arrays on a caller stream -- renders byte-identical
    images to the same sequence without them, on one render stream and on three."""
    monkeypatch.setenv("RT64_RENDER_STREAMS", str(streams))
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    rays = ray_rule.random_rays(sample_data, 51, 2000, floor_instance=3)
    images = (rt64.IMAGE_FINAL_RGBA8, rt64.IMAGE_OUTPUT_RGBA32F, rt64.IMAGE_INDIRECT_LIGHT_FILTERED, rt64.IMAGE_PRIMARY_HIT)

    def run(query):
        data = copy.copy(sample_data)
        s = sample_scene.Rt64Scene(rt64_lib, data, 96, 64, hip_device=0)
        hip = ray_rule.Hip()
        try:
            assert s.option("sync_present", 0)
            s.set_view_description(gi_samples=1, denoiser=True)
            assert s.option("denoiser_mode", 1)
            out = []
            st = hip.stream()
            n = len(rays)
            d_rays, d_hits, d_lay, d_rad, d_sky = hip.upload(rays), hip.alloc(3 * n * 32), hip.alloc(n * 16), hip.alloc(n * 64), hip.alloc(n * 32)
            for f in range(3):
                v = np.array(sample_data.view, dtype=np.float32).copy(); v[3, 0] += np.float32(0.05 * f)
                data.view = v
                s.draw()
                hits = rt64.trace_rays(rt64_lib, s.view, rays)
                if query:
                    rt64.trace_view_ray_radiance(rt64_lib, s.view, rays, 16, flags=CULL)
                    rt64.sky_view_pixels(rt64_lib, s.view, count=96 * 64)
                    assert rt64_lib.TraceViewRayLayersDevice(s.view, d_rays, None, 3, d_hits, d_lay, n, 0, st) == 1
                    assert rt64_lib.ComposeViewRayRadianceDevice(s.view, d_rays, d_hits, None, 3, d_rad, n, 0, st) == 1
                    assert rt64_lib.SkyViewRaysDevice(s.view, d_rays, d_sky, n, st) == 1
                out.append([s.readback(k).copy() for k in images] + [hits])
            return out
        finally:
            hip.close()
            s.close()
    a, b = run(False), run(True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert x.tobytes() == y.tobytes()
