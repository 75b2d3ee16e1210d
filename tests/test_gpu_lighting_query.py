"""Direct-light records of ray-query hits (RT64_LightViewRayHits, RT64_TraceViewRayLighting, include/rt64_lighting.h) on the GPU, held to the float64 rule of
tests/lighting_rule.py record by record (rules P1-P11), to the chain of sibling calls they replace, to the frame's own direct light (P8), and to
themselves: the forms agree byte for byte, nothing is written past the last record, counters follow count_traversal, bad calls are refused as P10 says and the
lights are those of the last drawn frame.

One run's lines of the first test are committed as profiles/lighting_rule_deviation.txt.
"""
import numpy as np
import pytest

import light_cases as LC
import lighting_cases as PC
import lighting_rule as R
import material_cases as MC
import material_rule as M
import ray_rule

pytestmark = pytest.mark.gpu

CULL, FIRST = ray_rule.CULL_BACK_FACING, ray_rule.ACCEPT_FIRST_HIT
BLOCKED = 0x2          # RT64_VISIBILITY_BLOCKED


def _open(rt64_lib, data, options=None, w=PC.W, h=PC.H):
    from sm64rt_legacy_renderer_amd import sample_scene
    options = dict(options or {})
    first = {k: options.pop(k) for k in ("generate_mipmaps",) if k in options}          # applies to textures created while it is set
    s = sample_scene.Rt64Scene(rt64_lib, data, w, h, hip_device=0, options=first)
    for k, v in options.items():
        assert s.option(k, v), k
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_rules = {}


def _rule(name, data, options, rays, hits, lods):
    """The rule on the device's own hits, once per case (the mutations of other tests evaluate their variants themselves)."""
    key = (name, _bits(hits)[:, :5].tobytes())
    if key not in _rules:
        _rules[key] = R.lighting(data, M.texture_levels(data, MC.mipmapped(options)), rays, hits, lods)
    return _rules[key]


@pytest.mark.parametrize("name", PC.NAMES)
def test_the_records_lie_within_the_rule(rt64_lib, oracle_lib, sample_data, name):
    """1.  Every case, with the LDS scene cache and without it (both instantiations of hit_light_kernel): direct, unshadowed and emitted within the bound on every
    decided record; flags, lightsAdmitted, lightsBlocked, instance and primitive exact; undecided records finite and at most 2 % of the real hits; the one-call form
    equal to walk + records byte for byte; each mutation assigned to the case leaves its bound against the device's records."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, heights = PC.make_case(sample_data, name)
    rays, lods = PC.rays_and_lods(data, seed, options, heights)
    got = {}
    for cache in (1, 0):
        s = _open(rt64_lib, data, dict(options, lds_cache=cache))
        try:
            s.draw()
            hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods)
            rec = rt64.light_hits(rt64_lib, s.view, rays, hits, lods)
            h2, rec2 = rt64.trace_lighting(rt64_lib, s.view, rays, lods)
            assert np.array_equal(_bits(h2), _bits(hits)) and np.array_equal(_bits(rec2), _bits(rec)), (name, cache)
            got[cache] = (hits, rec)
        finally:
            s.close()
    assert np.array_equal(_bits(got[0][0])[:, :5], _bits(got[1][0])[:, :5])
    hits = got[1][0]
    rule = _rule(name, data, options, rays, hits, lods)
    sh = R.shares(rule)
    for cache in (1, 0):
        ratios, exact = R.compare(rule, got[cache][1])
        print(R.report("%s lds_cache=%d" % (name, cache), rule, ratios, exact))
        assert exact.all(), (name, cache, np.nonzero(~exact)[0][:8].tolist())
        for k, r in ratios.items():
            assert (r <= 1.0).all(), (name, cache, k, float(r.max()), np.nonzero(~(r <= 1.0))[0][:8].tolist())
    need = PC.SHARES[name]
    assert all(a >= b for a, b in zip(sh[:5], need)), (sh, need)
    assert sh[5] <= PC.UNDECIDED_CAP, sh
    levels = M.texture_levels(data, MC.mipmapped(options))
    for mutation, where in PC.MUTATION_CASE.items():
        if where != name:
            continue
        wrong = R.lighting(data, levels, rays, hits, lods, mutate=mutation)
        ratios, exact = R.compare(wrong, got[1][1])
        out = ~exact
        for r in ratios.values():
            out |= ~(r <= 1.0)
        und = int((wrong["undecided"] | rule["undecided"]).sum())
        print("    mutation %-28s %4d of %4d of the device's records outside its bound (undecided with either rule: %d)" % (mutation, int(out.sum()), len(out), und))
        assert out.sum() > und, mutation


# ---- 2. the chain of calls the new one replaces ------------------------------------------------------------------------------------------------------------------

def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _host_chain(rt64_lib, view, data, rays, hits, lods):
    """Resolve, shade, build lights x hits shadow rays in float32 as P4-P6 say, RT64_TraceViewRayVisibility, combine with P5: what a host did before this call.
    -> (direct (N, 3) float32, blocked [N], admitted [N], rays per record)"""
    from sm64rt_legacy_renderer_amd import rt64
    surf = rt64.resolve_hits(rt64_lib, view, rays, hits)
    mat = rt64.shade_hits(rt64_lib, view, rays, hits, lods)
    n = len(rays)
    inp = R.scene_inputs(data)
    inst = hits.view(np.int32)[:, 3]
    real = (_bits(surf)[:, 3] & 1) != 0
    ids = np.where(real, inst, 0)
    field = lambda k: _f32([m[k] for m in inp["materials"]])[ids]
    mask = np.asarray([m["lightGroupMaskBits"] for m in inp["materials"]], dtype=np.uint32)[ids]
    P, N, S_, D = _f32(surf[:, 0:3]), _f32(mat[:, 4:7]), _f32(mat[:, 8:11]), _f32(rays[:, 4:7])
    inf, bias, expo = field("ignoreNormalFactor"), field("shadowRayBias"), field("specularExponent")
    one, zero = np.float32(1.0), np.float32(0.0)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    with np.errstate(all="ignore"):
        pw = lambda x, y: np.where(y == 0, one, np.power(x, y, dtype=np.float32)).astype(np.float32)
        direct = np.zeros((n, 3), dtype=np.float32); blocked = np.zeros(n, dtype=np.int64); count = np.zeros(n, dtype=np.int64)
        pending = []
        for l in inp["lights"]:
            lp = _f32(l["position"])[None]
            to = lp - P
            dist = np.sqrt(dot(to, to)).astype(np.float32)
            direction = (to * (one / dist)[:, None]).astype(np.float32)                      # len3_exact / normalize3_exact
            falloff = pw(np.maximum(one - dist * (one / np.float32(l["attenuationRadius"])), zero), np.float32(l["attenuationExponent"]))
            ndl = dot(N, direction)
            simple = falloff * np.maximum((ndl + inf * (one - ndl)) + np.float32(0.707106), zero) * np.float32(sum(_f32(l["diffuseColor"])))
            admitted = real & ((mask & np.uint32(l["groupBits"])) != 0) & (count < 16) & (simple > np.float32(1e-6))
            count += admitted
            lam = np.maximum(ndl, zero); lam = (lam + inf * (one - lam)) * falloff
            refl = -direction - N * (np.float32(2.0) * dot(N, -direction))[:, None]
            sp = pw(np.maximum(np.clip(dot(refl, -D) * falloff, zero, one), zero), expo)
            term = _f32(l["diffuseColor"])[None] * lam[:, None] + _f32(l["specularColor"])[None] * (S_ * sp[:, None])
            shadow = np.zeros((n, 8), dtype=np.float32)
            shadow[:, 0:3] = P; shadow[:, 3] = np.float32(0.1) + bias; shadow[:, 4:7] = direction; shadow[:, 7] = dist - np.float32(l["shadowOffset"])
            pending.append((admitted, term.astype(np.float32), shadow))
        every = np.ascontiguousarray(np.concatenate([p[2][p[0]] for p in pending])) if pending else np.zeros((0, 8), dtype=np.float32)
        vis = rt64.trace_visibility(rt64_lib, view, every) if len(every) else np.zeros((0, 4), dtype=np.float32)
        at = 0
        for admitted, term, _ in pending:
            k = int(admitted.sum())
            v = vis[at:at + k]; at += k
            direct[admitted] += term[admitted] * v[:, 0:1]
            blocked[admitted] += (_bits(v)[:, 1] & BLOCKED) != 0
    return direct, blocked, count, len(every)


@pytest.mark.parametrize("name", ["offsets", "veils"])
def test_one_call_equals_the_chain_of_siblings(rt64_lib, oracle_lib, sample_data, name):
    """2.  Positions from RT64_ResolveViewRayHits, normal and specular from RT64_ShadeViewRayHits, shadow rays built on the host in float32 and sent through
    RT64_TraceViewRayVisibility, combined on the host with P5: lightsAdmitted and lightsBlocked equal the chain's counts on every decided record (the device's
    shadow rays are IEEE products, sums, one square root and one division of the same float32 position, so the host's are the same bits wherever both admit the
    same lights: the K5 walk was not changed by being inlined), and the chain's direct lies within the rule's bound like the record's."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, heights = PC.make_case(sample_data, name)
    rays, lods = PC.rays_and_lods(data, seed, options, heights)
    s = _open(rt64_lib, data, options)
    try:
        s.draw()
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods)
        rec = rt64.light_hits(rt64_lib, s.view, rays, hits, lods)
        direct, blocked, admitted, sent = _host_chain(rt64_lib, s.view, data, rays, hits, lods)
    finally:
        s.close()
    rule = _rule(name, data, options, rays, hits, lods)
    decided = (rule["kind"] == 2) & ~rule["undecided"]
    ri = _bits(rec)
    same_lights = decided & (ri[:, 7] == admitted)
    differ = decided & same_lights & (ri[:, 11] != blocked)
    v, e = rule["direct"]
    host_ratio = np.where(decided[:, None], np.abs(direct.astype(np.float64) - v) / e, 0.0)
    pair = np.where(decided[:, None], np.abs(direct.astype(np.float64) - rec[:, 0:3].astype(np.float64)) / (2.0 * e), 0.0)
    print("%-8s decided %4d  shadow rays sent %5d  admitted differently %d  lightsBlocked differs %d  chain / bound max %.3f  |chain - record| / 2 bound max %.3f" %
          (name, int(decided.sum()), sent, int((decided & ~same_lights).sum()), int(differ.sum()), host_ratio.max(), pair.max()))
    assert decided.sum() > 300 and sent > 1000
    assert not (decided & ~same_lights).any() and not differ.any()
    assert (host_ratio <= 1.0).all() and (pair <= 1.0).all()


# ---- 3. the frame (P8) ------------------------------------------------------------------------------------------------------------------------------------------------

def _frame_pixels():
    return np.stack(np.meshgrid(np.arange(LC.W), np.arange(LC.H), indexing="xy"), axis=-1).reshape(-1, 2)


def _oracle_quantisation(data, view, rays):
    """How far a frame's stored direct light lies from the rule at unquantised inputs, measured where no GPU is involved: the oracle's DIRECT_LIGHT_RAW against
    lighting_rule on the oracle's own hits of the pixels' camera rays.  -> (largest |difference| over the pixels both rules decide and whose candidates are all
    drawn, the rule's records, those pixels)"""
    from oracle import oracle_py
    o = oracle_py.OracleScene(data)
    try:
        ref = o.render(LC.W, LC.H, images=True, diSamples=view["di_samples"], maxLights=view["max_lights"])
        hits = ray_rule.trace(o, rays, CULL)
    finally:
        o.close()
    rule = R.lighting(data, M.texture_levels(data), rays, hits)
    _, _, decided, info = LC.run_rule(data, view, 0, ref["shadingPosition"], ref["shadingNormal"], ref["shadingSpecular"], ref["instanceId"])
    held = (decided & (info["draws"] == info["candidates"])).reshape(-1) & (rule["kind"] == 2) & ~rule["undecided"] & (ref["instanceId"].reshape(-1) == rule["instance"])
    total = rule["direct"][0] + rule["emitted"][0]
    diff = np.abs(ref["directLight"].reshape(-1, 4)[:, :3].astype(np.float64) - total)
    return float(diff[held].max()), rule, held


@pytest.mark.parametrize("name", ["one", "offsets", "material"])
def test_camera_rays_agree_with_the_frame(rt64_lib, oracle_lib, sample_data, name):
    """3.  di_samples = 0, max_lights = 16, every G-buffer image written: for the camera ray of every pixel RT64_TraceViewRayLighting names RT64_IMAGE_PRIMARY_HIT's
    instance, and direct + emitted is RT64_IMAGE_DIRECT_LIGHT_RAW up to what the frame's quantised inputs (SNORM16 normal, f16 store) do to it.  That is no
    property of the rule, so it is measured on the oracle: its DIRECT_LIGHT_RAW against the rule at unquantised inputs, the largest difference over the pixels
    held; the device's frame and the device's records may differ by that plus the rule's bound."""
    from sm64rt_legacy_renderer_amd import rt64
    data, view = PC.frame_case(sample_data, name)
    rays = ray_rule.camera_rays(data, LC.W, LC.H, _frame_pixels())
    tolerance, rule, held = _oracle_quantisation(data, view, rays)
    s = _open(rt64_lib, data, {"lean_frames": 0}, LC.W, LC.H)
    try:
        s.set_view_description(di_samples=view["di_samples"], max_lights=view["max_lights"])
        s.draw()
        shown = s.readback(rt64.IMAGE_PRIMARY_HIT); raw = s.readback(rt64.IMAGE_DIRECT_LIGHT_RAW)
        hits, rec = rt64.trace_lighting(rt64_lib, s.view, rays, None, CULL)
    finally:
        s.close()
    shown = np.where(shown[..., 3] == 0xFFFFFFFF, -1, (shown[..., 3] >> 24).astype(np.int64)).reshape(-1)
    mine = rec.view(np.int32)[:, 12]
    same = held & (mine == shown) & (mine == rule["instance"])
    total = rec[:, 0:3].astype(np.float64) + rec[:, 8:11].astype(np.float64)
    diff = np.abs(raw.reshape(-1, 4)[:, :3].astype(np.float64) - total).max(axis=1)
    bound = (rule["direct"][1] + rule["emitted"][1]).max(axis=1)
    shaded = int((shown >= 0).sum())
    print("%-8s shaded %4d held %4d left out %.4f  oracle's largest difference %.3e  device's %.3e" % (name, shaded, int(same.sum()), 1.0 - same.sum() / shaded, tolerance, diff[same].max()))
    assert shaded > 1500 and (held & (mine != shown)).sum() == 0
    assert 1.0 - same.sum() / shaded <= 0.02
    assert (diff[same] <= tolerance + bound[same]).all(), (float(diff[same].max()), tolerance)


# ---- 4. forms, sizes, counters, refusals, lifetime ---------------------------------------------------------------------------------------------------------------------

def test_forms_sizes_and_the_end_of_the_array(rt64_lib, sample_data):
    """4.  Host arrays, device arrays on the device's stream and on a caller stream: the same records; lods = NULL is an array of zeros; counts 1, 63, 64, 65, 257
    and RT_GRID_BLOCKS x RT_BLOCK + 65 (the grid-stride loop) equal the prefix of one big call, with the guard words behind the last record untouched; misses and
    bad hits give P1's records."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, heights = PC.make_case(sample_data, "veils")
    s = _open(rt64_lib, data, {"generate_mipmaps": 1})
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = PC.rays_and_lods(data, seed, options, heights)[0]
        lods = MC.lods(seed, len(rays), True)
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods)
        hb = _bits(hits)
        hb[3, 3] = 1000; hb[4, 3] = 0; hb[4, 4] = 0x7FFFFFFF; hb[5, 3] = 0x80000001         # P1: instance past the end, primitive past the end, a negative instance (a miss)
        host = rt64.light_hits(rt64_lib, s.view, rays, hits, lods)
        b = _bits(host)
        miss = b[:, 12] == 0xFFFFFFFF
        assert (b[miss][:, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15]] == 0).all() and (b[miss, 13] == 0xFFFFFFFF).all() and set(b[miss, 3].tolist()) <= {0, R.BAD_HIT}
        assert b[3, 3] == R.BAD_HIT and b[4, 3] == R.BAD_HIT and b[5, 3] == 0 and miss[3] and miss[4] and miss[5]
        assert (~miss).sum() > 500 and (((host[:, 0:3] < host[:, 4:7]).any(axis=1)) & ~miss).sum() > 100          # dimmed by a layer
        d_rays, d_hits, d_lods = hip.upload(rays), hip.upload(hits), hip.upload(lods)
        for l, d_l in ((lods, d_lods), (None, None)):
            want = host if l is not None else rt64.light_hits(rt64_lib, s.view, rays, hits, None)
            for st in (None, hip.stream()):
                d_out = hip.alloc(want.nbytes)
                assert rt64_lib.LightViewRayHitsDevice(s.view, d_rays, d_hits, d_l, d_out, len(rays), st) == 1, rt64_lib.last_error()
                if st:
                    assert hip.h.hipStreamSynchronize(st) == 0
                assert np.array_equal(_bits(hip.download(d_out, want)), _bits(want))
            if l is None:
                assert np.array_equal(_bits(rt64.light_hits(rt64_lib, s.view, rays, hits, np.zeros(len(rays), dtype=np.float32))), _bits(want))
        big = 2048 * 256 + 65
        reps = -(-(big + 300) // len(rays))
        rng = np.random.default_rng(6)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(reps - 1)])          # later repetitions shuffled: waves mix instances
        many, many_hits, many_lods = np.ascontiguousarray(rays[order]), np.ascontiguousarray(hits[order]), np.ascontiguousarray(lods[order])
        whole = _bits(rt64.light_hits(rt64_lib, s.view, many, many_hits, many_lods))          # host form: chunks of 2^18
        assert np.array_equal(whole, _bits(host)[order])                                        # a record does not depend on its place or its neighbours
        d_rays, d_hits, d_lods = hip.upload(many), hip.upload(many_hits), hip.upload(many_lods)
        guard = np.full((len(many), 16), 0xABABABAB, dtype=np.uint32)
        for count in (1, 63, 64, 65, 257, big):
            d_guard = hip.upload(guard[:count + 258])
            assert rt64_lib.LightViewRayHitsDevice(s.view, d_rays, d_hits, d_lods, d_guard, count, None) == 1, rt64_lib.last_error()
            out = hip.download(d_guard, guard[:count + 258])
            assert np.array_equal(out[:count], whole[:count]) and (out[count:] == 0xABABABAB).all(), count
    finally:
        hip.close()
        s.close()


def test_counters_follow_count_traversal(rt64_lib, sample_data):
    """5.  P9: nodesVisited and trianglesTested are 0 without count_traversal; with it, non-zero exactly on the records that walked a shadow ray into the scene
    box, and the floats do not change."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, heights = PC.make_case(sample_data, "masks")
    rays, lods = PC.rays_and_lods(data, seed, options, heights)
    s = _open(rt64_lib, data)
    try:
        s.draw()
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        a = _bits(rt64.light_hits(rt64_lib, s.view, rays, hits))
        assert not a[:, 14:16].any()
        assert s.option("count_traversal", 1)
        s.draw()
        hits2 = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        b = _bits(rt64.light_hits(rt64_lib, s.view, rays, hits2))
    finally:
        s.close()
    assert np.array_equal(a[:, :14], b[:, :14])
    unlit = (b[:, 3] & R.UNLIT) != 0
    lit = (b[:, 7] > 0)
    assert unlit.sum() > 50 and not b[unlit][:, 14:16].any() and not b[b[:, 12] == 0xFFFFFFFF][:, 14:16].any()
    assert lit.sum() > 100 and (b[lit, 14] > 0).all() and (b[b[:, 11] > 0, 15] > 0).all()


def test_refusals_and_the_lights_of_the_last_frame(rt64_lib, sample_data):
    """6.  P10: every refusal returns 0 with a message that names the function; count = 0 succeeds and touches nothing; RT64_SetSceneLights after the draw changes
    nothing until the next draw."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, heights = PC.make_case(sample_data, "material")
    rays, _ = PC.rays_and_lods(data, seed, options, heights)
    rays = np.ascontiguousarray(rays[:600])
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    R_ = rt64_lib
    try:
        hits = np.zeros((len(rays), 8), dtype=np.float32); out = np.full((len(rays), 16), 0xABABABAB, dtype=np.uint32)
        d_rays, d_hits, d_out, d_lods = hip.upload(rays), hip.upload(hits), hip.alloc(out.nbytes), hip.upload(np.zeros(len(rays), dtype=np.float32))
        Lh, Ld, Lt = "RT64_LightViewRayHits", "RT64_LightViewRayHitsDevice", "RT64_TraceViewRayLighting"

        def refused(word, fn, call):
            ok = call()
            assert ok == 0 and fn + ":" in R_.last_error() and word in R_.last_error(), (ok, R_.last_error())

        def all_refused(word):
            refused(word, Lh, lambda: R_.LightViewRayHits(s.view, rays.ctypes.data, hits.ctypes.data, None, out.ctypes.data, len(rays)))
            refused(word, Ld, lambda: R_.LightViewRayHitsDevice(s.view, d_rays, d_hits, None, d_out, 4, None))
            refused(word, Lt, lambda: R_.TraceViewRayLighting(s.view, rays.ctypes.data, None, None, out.ctypes.data, len(rays), 0))
        all_refused("draw")                                                               # before the first frame
        s.draw()
        hits = rt64.trace_rays_alpha(R_, s.view, rays)
        want = rt64.light_hits(R_, s.view, rays, hits)
        assert R_.LightViewRayHits(s.view, rays.ctypes.data, hits.ctypes.data, None, out.ctypes.data, 0) == 1
        assert R_.TraceViewRayLighting(s.view, rays.ctypes.data, None, None, out.ctypes.data, 0, 0) == 1
        refused("NULL", Lh, lambda: R_.LightViewRayHits(s.view, None, hits.ctypes.data, None, out.ctypes.data, 4))
        refused("NULL", Lh, lambda: R_.LightViewRayHits(s.view, rays.ctypes.data, None, None, out.ctypes.data, 4))
        refused("NULL", Lh, lambda: R_.LightViewRayHits(s.view, rays.ctypes.data, hits.ctypes.data, None, None, 4))
        refused("NULL view", Lh, lambda: R_.LightViewRayHits(None, rays.ctypes.data, hits.ctypes.data, None, out.ctypes.data, 4))
        refused("NULL", Lt, lambda: R_.TraceViewRayLighting(s.view, rays.ctypes.data, None, None, None, 4, 0))
        refused("NULL", Ld, lambda: R_.LightViewRayHitsDevice(s.view, d_rays, None, None, d_out, 4, None))
        refused("unknown flags", Lt, lambda: R_.TraceViewRayLighting(s.view, rays.ctypes.data, None, None, out.ctypes.data, 4, FIRST))
        refused("unknown flags", Lt, lambda: R_.TraceViewRayLighting(s.view, rays.ctypes.data, None, None, out.ctypes.data, 4, 0x4))
        for a, h, l, o in ((d_rays + 4, d_hits, None, d_out), (d_rays, d_hits + 8, None, d_out), (d_rays, d_hits, None, d_out + 4), (d_rays, d_hits, d_lods + 2, d_out)):
            refused("aligned", Ld, lambda: R_.LightViewRayHitsDevice(s.view, a, h, l, o, 4, None))
        assert R_.LightViewRayHitsDevice(s.view, d_rays, d_hits, d_lods + 4, d_out, 4, None) == 1          # lods need 4-byte alignment only
        assert (out == 0xABABABAB).all()
        m = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], m.vertices, m.indices)
        all_refused("RT64_SetMesh")
        s.draw()
        assert np.array_equal(_bits(rt64.light_hits(R_, s.view, rays, hits)), _bits(want))
        # the lights are the last drawn frame's
        dark = (rt64.LIGHT * 1)(LC._light(data.lights[0], (0.0, 50.0, 0.0), (0.0, 0.0, 0.0)))
        R_.SetSceneLights(s.scene, dark, 1)
        assert np.array_equal(_bits(rt64.light_hits(R_, s.view, rays, hits)), _bits(want))
        assert (want[:, 0:3] > 0).any()
        stock = list(data.lights); data.lights = [dark[0]]; s._lights = dark
        s.draw()
        now = rt64.light_hits(R_, s.view, rays, hits)
        data.lights = stock
        assert not now[:, 0:3].any() and not _bits(now)[:, 7].any() and np.array_equal(_bits(now)[:, 8:11], _bits(want)[:, 8:11])
    finally:
        hip.close()
        s.close()
