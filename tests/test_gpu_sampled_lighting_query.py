"""Sampled direct-light records of ray-query hits (RT64_SampleViewRayLights, RT64_TraceViewRaySampledLights, include/rt64_sampled_lighting.h) on the GPU, held
to the float64 rule of tests/sampled_lighting_rule.py record by record (rules J1-J11), to the frame's own direct light (J10), to a twin session drawn
up to the key's frame count, to RT64_LightViewRayHits where the overrides draw every candidate, and to themselves: the forms agree byte for byte, nothing is
written past the last record, counters follow count_traversal, bad calls are refused as J11 says and the lights are those of the last drawn frame.

One run's lines are committed as profiles/sampled_lighting_rule_deviation.txt.
"""
import ctypes as C

import numpy as np
import pytest

import light_cases as LC
import lighting_rule as P
import material_rule as M
import ray_rule
import sampled_lighting_cases as SC
import sampled_lighting_rule as R

pytestmark = pytest.mark.gpu

CULL, FIRST = ray_rule.CULL_BACK_FACING, ray_rule.ACCEPT_FIRST_HIT


def _open(rt64_lib, data, view, frames, options=None):
    """A session of the case's scene at 88 x 72 with `frames` frames drawn under the view description."""
    from sm64rt_legacy_renderer_amd import sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, data, SC.W, SC.H, hip_device=0)
    try:
        for k, v in (options or {}).items():
            assert s.option(k, v), k
        s.set_view_description(**view)
        for _ in range(frames):
            s.draw()
    except Exception:
        s.close()
        raise
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _popcount(x):
    return np.array([bin(int(v)).count("1") for v in x], dtype=np.int64)


# ---- 1. the rule, record by record ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SC.NAMES)
def test_the_records_lie_within_the_rule(rt64_lib, oracle_lib, sample_data, name):
    """1.  Every case, with the LDS scene cache and without it (both instantiations of hit_sampled_light_kernel): direct, unshadowed and emitted within the bound on
    every decided record; flags, lightsAdmitted, drawn, instance and primitive exact; undecided records finite and at most 2 % of the real hits; the one-call form
    equal to walk + records byte for byte; each wrong reading assigned to the case leaves its bound against the device's records."""
    from sm64rt_legacy_renderer_amd import rt64
    data, view, frames = SC.make_case(sample_data, name)
    rays, keys = SC.rays_and_keys(data, name)
    over = SC.OVERRIDES.get(name)
    got = {}
    for cache in (1, 0):
        s = _open(rt64_lib, data, view, frames, {"lds_cache": cache})
        try:
            hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
            rec = rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys)
            h2, rec2 = rt64.trace_sampled_lighting(rt64_lib, s.view, rays, None, keys)
            assert np.array_equal(_bits(h2), _bits(hits)) and np.array_equal(_bits(rec2), _bits(rec)), (name, cache)
            got[cache] = (hits, rec, rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys, *over) if over else None)
        finally:
            s.close()
    assert np.array_equal(_bits(got[0][0])[:, :5], _bits(got[1][0])[:, :5])
    hits = got[1][0]
    levels, frame = M.texture_levels(data), SC.frame_of(view, frames)
    rule = R.sampled(data, levels, rays, hits, keys, frame)
    sh = R.shares(rule)
    for cache in (1, 0):
        ratios, exact = R.compare(rule, got[cache][1])
        print(R.report("%s lds_cache=%d" % (name, cache), rule, ratios, exact))
        assert exact.all(), (name, cache, np.nonzero(~exact)[0][:8].tolist())
        for k, r in ratios.items():
            assert (r <= 1.0).all(), (name, cache, k, float(r.max()), np.nonzero(~(r <= 1.0))[0][:8].tolist())
    assert all(a >= b for a, b in zip(sh[:3], SC.SHARES[name])), (sh, SC.SHARES[name])
    assert sh[3] <= SC.UNDECIDED_CAP, sh
    overridden = None
    if over:          # 4a.  J4: the same records with every candidate drawn and no disc follow the rule as well
        overridden = R.sampled(data, levels, rays, hits, keys, frame, max_lights=over[0], di_samples=over[1])
        for cache in (1, 0):
            ratios, exact = R.compare(overridden, got[cache][2])
            print(R.report("%s {%d, %d} lds_cache=%d" % (name, over[0], over[1], cache), overridden, ratios, exact))
            assert exact.all() and all((r <= 1.0).all() for r in ratios.values()), (name, cache)
    for mutation, where in SC.MUTATION_CASE.items():
        if where != name:
            continue
        if mutation == "overrides_ignored":
            right, wrong, device = overridden, R.sampled(data, levels, rays, hits, keys, frame, max_lights=over[0], di_samples=over[1], mutate=mutation), got[1][2]
        else:
            right, wrong, device = rule, R.sampled(data, levels, rays, hits, keys, frame, mutate=mutation), got[1][1]
        out = R.outside(wrong, device)
        und = int((wrong["undecided"] | right["undecided"]).sum())
        print("    mutation %-22s %4d of %4d of the device's records outside its bound (undecided with either rule: %d)" % (mutation, int(out.sum()), len(out), und))
        assert out.sum() > und, mutation


# ---- 2. the frame (J10) ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["four", "pick-one", "radius-4", "noise"])
def test_camera_rays_with_default_keys_agree_with_the_frame(rt64_lib, oracle_lib, sample_data, name):
    """2.  lean_frames = 0, every G-buffer image written.  The rays of RT64_GenerateViewCameraRays, their RT64_TraceViewRaysAlpha hits, keys = NULL, sampling = NULL:
    |direct + emitted - DIRECT_LIGHT_RAW| <= L8 at the stored inputs + the record's own bound + |rule(stored) - rule(unquantised)|, every term the rules'.  Left out:
    pixels either rule leaves undecided, pixels whose hit is not the frame's instance, and pixels whose drawn mask differs between stored and unquantised inputs
    (SNORM16 / f16 quantisation can move a walk decision); at most 2 % of the shaded pixels."""
    from sm64rt_legacy_renderer_amd import rt64
    data, view, frames = SC.make_case(sample_data, name)
    s = _open(rt64_lib, data, view, frames, {"lean_frames": 0})
    try:
        img = {k: s.readback(getattr(rt64, "IMAGE_" + k)) for k in ("SHADING_POSITION", "SHADING_NORMAL", "SHADING_SPECULAR", "INSTANCE_ID", "DIRECT_LIGHT_RAW")}
        rays = rt64.camera_rays(rt64_lib, s.view, None, SC.W * SC.H, differentials=False)
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        rec = rt64.sample_lighting(rt64_lib, s.view, rays, hits)
    finally:
        s.close()
    frame = SC.frame_of(view, frames)
    value, bound, decided, drawn = R.at_gbuffer(data, img["SHADING_POSITION"], img["SHADING_NORMAL"], img["SHADING_SPECULAR"], img["INSTANCE_ID"],
                                                LC.rule_inputs(data)["camera"], frame)
    rule = R.sampled(data, M.texture_levels(data), rays, hits, None, frame)
    shown = img["INSTANCE_ID"].reshape(-1)
    lit = shown >= 0
    ri = _bits(rec)
    ratios, exact = R.compare(rule, rec)
    assert exact.all() and all((r <= 1.0).all() for r in ratios.values())
    held = lit & decided.reshape(-1) & (rule["kind"] == 2) & ~rule["undecided"] & (rule["instance"] == shown) & (rule["drawn"] == drawn.reshape(-1)) & (ri[:, 11] == drawn.reshape(-1))
    total = rec[:, 0:3].astype(np.float64) + rec[:, 8:11].astype(np.float64)
    diff = np.abs(img["DIRECT_LIGHT_RAW"].reshape(-1, 4)[:, :3].astype(np.float64) - total)
    mine = rule["direct"][0] + rule["emitted"][0]
    allowed = bound.reshape(-1, 3) + rule["direct"][1] + rule["emitted"][1] + np.abs(value.reshape(-1, 3) - mine)
    left_out = 1.0 - held.sum() / lit.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / allowed)[held]
    print("%-9s shaded %4d held %4d left out %.4f  |record - frame| / allowed max %.3f mean %.4f  largest allowed %.2e  redrawn %d" %
          (name, int(lit.sum()), int(held.sum()), left_out, ratio.max(), ratio.mean(), allowed[held].max(), int(((ri[:, 11] >> 16) != 0).sum())))
    assert lit.sum() > 1500 and left_out <= 0.02
    assert (ratio <= 1.0).all()


# ---- 3. the key is the pixel and the frame ----------------------------------------------------------------------------------------------------------------------------------

def test_a_key_equals_the_twin_session_drawn_up_to_its_frame(rt64_lib, sample_data):
    """3.  Records with key.frame = f on a view whose last frame had count 0 are byte-equal to keys = NULL records of a twin session drawn up to count f: the same
    scene, the same pixels, f = 1, 2, 5."""
    from sm64rt_legacy_renderer_amd import rt64
    data, view, _ = SC.make_case(sample_data, "four")
    n = SC.W * SC.H
    keyed = {}
    s = _open(rt64_lib, data, view, 1)
    try:
        rays = rt64.camera_rays(rt64_lib, s.view, None, n, differentials=False)
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        keys = np.zeros((n, 4), dtype=np.uint32); keys[:, 0] = np.arange(n) % SC.W; keys[:, 1] = np.arange(n) // SC.W
        for f in (0, 1, 2, 5):
            keys[:, 2] = f
            keyed[f] = _bits(rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys))
        assert np.array_equal(keyed[0], _bits(rt64.sample_lighting(rt64_lib, s.view, rays, hits)))          # keys = NULL is (i % width, i / width, frameCount)
    finally:
        s.close()
    assert not np.array_equal(keyed[0], keyed[1]) and not np.array_equal(keyed[1], keyed[2])
    s = _open(rt64_lib, data, view, 1)
    try:
        drawn = 1
        for f in (1, 2, 5):
            while drawn < f + 1:
                s.draw(); drawn += 1
            twin = _bits(rt64.sample_lighting(rt64_lib, s.view, rays, rt64.trace_rays_alpha(rt64_lib, s.view, rays)))
            assert np.array_equal(twin, keyed[f]), f
    finally:
        s.close()


# ---- 4. overrides ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_every_candidate_at_its_centre_is_the_unsampled_query(rt64_lib, oracle_lib, sample_data):
    """4b.  {16, 0} on "four", drawn with {3, 2}: on records whose drawn high half is 0 every candidate is lit exactly once at its centre, which is what
    RT64_LightViewRayHits sums in list order: lightsAdmitted is equal, popcount(drawn & 0xFFFF) = lightsAdmitted, and unshadowed lies within the summed bounds
    of the two rules (the order of the sum differs: the draws' against the list's)."""
    from sm64rt_legacy_renderer_amd import rt64
    data, view, frames = SC.make_case(sample_data, "four")
    rays, keys = SC.rays_and_keys(data, "four")
    s = _open(rt64_lib, data, view, frames)
    try:
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        rec = rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys, 16, 0)
        plain = rt64.light_hits(rt64_lib, s.view, rays, hits)
        same = rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys, 3, 2)
        assert np.array_equal(_bits(same), _bits(rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys)))          # the frame's own values, spelled out
        assert np.array_equal(_bits(rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys, -1, 2)), _bits(same))
    finally:
        s.close()
    levels = M.texture_levels(data)
    mine = R.sampled(data, levels, rays, hits, keys, SC.frame_of(view, frames), max_lights=16, di_samples=0)
    theirs = P.lighting(data, levels, rays, hits)
    ri, pi = _bits(rec), _bits(plain)
    once = (mine["kind"] == 2) & ~mine["undecided"] & ~theirs["undecided"] & ((ri[:, 11] >> 16) == 0)
    assert once.sum() > 1000
    assert np.array_equal(ri[once, 7], pi[once, 7]) and np.array_equal(_popcount(ri[once, 11] & 0xFFFF), ri[once, 7].astype(np.int64))
    diff = np.abs(rec[:, 4:7].astype(np.float64) - plain[:, 4:7].astype(np.float64))
    allowed = mine["unshadowed"][1] + theirs["unshadowed"][1]
    print("four {16, 0}: %d records lit once per candidate; |unshadowed - RT64_LightViewRayHits'| / summed bounds max %.3f" % (int(once.sum()), (diff[once] / allowed[once]).max()))
    assert (diff[once] <= allowed[once]).all()


# ---- 5. forms, sizes, counters, refusals, lifetime -------------------------------------------------------------------------------------------------------------------------

def test_forms_sizes_and_the_end_of_the_array(rt64_lib, sample_data):
    """5a.  Host arrays, device arrays on the device's stream and on a caller stream: the same records, with keys and without, with overrides and without; lods =
    NULL is an array of zeros; counts 1, 63, 64, 65, 257 and one staging chunk + 65 equal the prefix of one big call, with the guard words behind the last record
    untouched; misses and bad hits give J1's records."""
    from sm64rt_legacy_renderer_amd import rt64
    data, view, frames = SC.make_case(sample_data, "noise")
    rays, keys = SC.rays_and_keys(data, "noise")
    s = _open(rt64_lib, data, view, frames)
    hip = ray_rule.Hip()
    try:
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        hb = _bits(hits)
        live = np.nonzero(hits.view(np.int32)[:, 3] >= 0)[0]
        a, b, c = live[:3]
        hb[a, 3] = 1000; hb[b, 4] = 0x7FFFFFFF; hb[c, 3] = 0x80000001         # J1: instance past the end, primitive past the end, a negative instance (a miss)
        host = rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys)
        w = _bits(host)
        miss = w[:, 12] == 0xFFFFFFFF
        assert (w[miss][:, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15]] == 0).all() and (w[miss, 13] == 0xFFFFFFFF).all() and set(w[miss, 3].tolist()) <= {0, R.BAD_HIT}
        assert w[a, 3] == R.BAD_HIT and w[b, 3] == R.BAD_HIT and w[c, 3] == 0 and miss[a] and miss[b] and miss[c]
        assert (~miss).sum() > 1000 and (((host[:, 0:3] < host[:, 4:7]).any(axis=1)) & ~miss).sum() > 100          # in some shadow
        assert np.array_equal(_bits(rt64.sample_lighting(rt64_lib, s.view, rays, hits, np.zeros(len(rays), dtype=np.float32), keys)), w)          # lods = NULL is level 0
        d_rays, d_hits, d_keys, d_lods = hip.upload(rays), hip.upload(hits), hip.upload(keys), hip.upload(np.zeros(len(rays), dtype=np.float32))
        sampling = rt64.LIGHT_SAMPLING(5, 3, 0, 0)
        for k, d_k, count in ((keys, d_keys, len(rays)), (None, None, len(rays))):          # (3288 records: fewer than the frame's 6336 pixels)
            for p in (None, C.addressof(sampling)):
                want = _bits(rt64.sample_lighting(rt64_lib, s.view, rays[:count], hits[:count], None, k[:count] if k is not None else None, *((5, 3) if p else ())))
                for l in (None, d_lods):
                    for st in (None, hip.stream()):
                        d_out = hip.alloc(want.nbytes)
                        assert rt64_lib.SampleViewRayLightsDevice(s.view, d_rays, d_hits, l, d_k, p, d_out, count, st) == 1, rt64_lib.last_error()
                        if st:
                            assert hip.h.hipStreamSynchronize(st) == 0
                        assert np.array_equal(hip.download(d_out, want), want)
        assert not np.array_equal(w, _bits(rt64.sample_lighting(rt64_lib, s.view, rays, hits)))   # (the keys matter)
        big = (1 << 18) + 65
        reps = -(-(big + 300) // len(rays))
        rng = np.random.default_rng(6)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(reps - 1)])          # later repetitions shuffled: waves mix instances and keys
        many, many_hits, many_keys = np.ascontiguousarray(rays[order]), np.ascontiguousarray(hits[order]), np.ascontiguousarray(keys[order])
        whole = _bits(rt64.sample_lighting(rt64_lib, s.view, many, many_hits, None, many_keys))          # host form: chunks of 2^18
        assert np.array_equal(whole, w[order])                                                          # a record does not depend on its place or its neighbours
        d_rays, d_hits, d_keys = hip.upload(many), hip.upload(many_hits), hip.upload(many_keys)
        guard = np.full((len(many), 16), 0xABABABAB, dtype=np.uint32)
        for count in (1, 63, 64, 65, 257, big):
            d_guard = hip.upload(guard[:count + 258])
            assert rt64_lib.SampleViewRayLightsDevice(s.view, d_rays, d_hits, None, d_keys, None, d_guard, count, None) == 1, rt64_lib.last_error()
            out = hip.download(d_guard, guard[:count + 258])
            assert np.array_equal(out[:count], whole[:count]) and (out[count:] == 0xABABABAB).all(), count
    finally:
        hip.close()
        s.close()


def test_counters_follow_count_traversal(rt64_lib, sample_data):
    """5b.  J11 / P9: nodesVisited and trianglesTested are 0 without count_traversal; with it, non-zero on the records that drew a light, and the other words do
    not change."""
    from sm64rt_legacy_renderer_amd import rt64
    data, view, frames = SC.make_case(sample_data, "material")
    rays, keys = SC.rays_and_keys(data, "material")
    s = _open(rt64_lib, data, view, frames)
    try:
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        a = _bits(rt64.sample_lighting(rt64_lib, s.view, rays, hits, None, keys))
        assert not a[:, 14:16].any()
        assert s.option("count_traversal", 1)
        s.draw()
        hits2 = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        b = _bits(rt64.sample_lighting(rt64_lib, s.view, rays, hits2, None, keys))
    finally:
        s.close()
    assert np.array_equal(a[:, :14], b[:, :14])
    lit = b[:, 11] != 0
    assert lit.sum() > 1000 and (b[lit, 14] > 0).all() and not b[b[:, 12] == 0xFFFFFFFF][:, 14:16].any()
    assert (b[:, 15] > 0).sum() > 300


def test_refusals_and_the_lights_of_the_last_frame(rt64_lib, sample_data):
    """5c.  J11: every refusal returns 0 with a message that names the function; count = 0 succeeds and touches nothing; RT64_SetSceneLights after the draw changes
    nothing until the next draw."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    data, view, frames = SC.make_case(sample_data, "material")
    rays, keys = SC.rays_and_keys(data, "material")
    rays, keys = np.ascontiguousarray(rays[-600:]), np.ascontiguousarray(keys[-600:])
    s = sample_scene.Rt64Scene(rt64_lib, data, SC.W, SC.H, hip_device=0)
    hip = ray_rule.Hip()
    R_ = rt64_lib
    try:
        s.set_view_description(**view)
        hits = np.zeros((len(rays), 8), dtype=np.float32); out = np.full((len(rays), 16), 0xABABABAB, dtype=np.uint32)
        d_rays, d_hits, d_keys, d_out, d_lods = hip.upload(rays), hip.upload(hits), hip.upload(keys), hip.alloc(out.nbytes), hip.upload(np.zeros(len(rays), dtype=np.float32))
        Sh, Sd, St = "RT64_SampleViewRayLights", "RT64_SampleViewRayLightsDevice", "RT64_TraceViewRaySampledLights"
        r_, h_, k_, o_ = rays.ctypes.data, hits.ctypes.data, keys.ctypes.data, out.ctypes.data

        def refused(word, fn, call):
            ok = call()
            assert ok == 0 and fn + ":" in R_.last_error() and word in R_.last_error(), (ok, R_.last_error())

        def all_refused(word):
            refused(word, Sh, lambda: R_.SampleViewRayLights(s.view, r_, h_, None, k_, None, o_, len(rays)))
            refused(word, Sd, lambda: R_.SampleViewRayLightsDevice(s.view, d_rays, d_hits, None, d_keys, None, d_out, 4, None))
            refused(word, St, lambda: R_.TraceViewRaySampledLights(s.view, r_, None, None, k_, None, o_, len(rays), 0))
        all_refused("draw")                                                               # before the first frame
        s.draw()
        hits = rt64.trace_rays_alpha(R_, s.view, rays); h_ = hits.ctypes.data
        want = rt64.sample_lighting(R_, s.view, rays, hits, None, keys)
        assert R_.SampleViewRayLights(s.view, r_, h_, None, k_, None, o_, 0) == 1
        assert R_.TraceViewRaySampledLights(s.view, r_, None, None, k_, None, o_, 0, 0) == 1
        refused("NULL", Sh, lambda: R_.SampleViewRayLights(s.view, None, h_, None, k_, None, o_, 4))
        refused("NULL", Sh, lambda: R_.SampleViewRayLights(s.view, r_, None, None, k_, None, o_, 4))
        refused("NULL", Sh, lambda: R_.SampleViewRayLights(s.view, r_, h_, None, k_, None, None, 4))
        refused("NULL view", Sh, lambda: R_.SampleViewRayLights(None, r_, h_, None, k_, None, o_, 4))
        refused("NULL", St, lambda: R_.TraceViewRaySampledLights(s.view, r_, None, None, k_, None, None, 4, 0))
        refused("NULL", Sd, lambda: R_.SampleViewRayLightsDevice(s.view, d_rays, None, None, d_keys, None, d_out, 4, None))
        refused("unknown flags", St, lambda: R_.TraceViewRaySampledLights(s.view, r_, None, None, k_, None, o_, 4, FIRST))
        refused("unknown flags", St, lambda: R_.TraceViewRaySampledLights(s.view, r_, None, None, k_, None, o_, 4, 0x4))
        for a, h, k, l, o in ((d_rays + 4, d_hits, d_keys, None, d_out), (d_rays, d_hits + 8, d_keys, None, d_out), (d_rays, d_hits, d_keys + 4, None, d_out),
                              (d_rays, d_hits, d_keys, None, d_out + 4), (d_rays, d_hits, d_keys, d_lods + 2, d_out)):
            refused("aligned", Sd, lambda: R_.SampleViewRayLightsDevice(s.view, a, h, l, k, None, o, 4, None))
        assert R_.SampleViewRayLightsDevice(s.view, d_rays, d_hits, d_lods + 4, d_keys, None, d_out, 4, None) == 1          # lods need 4-byte alignment only
        # J3: keys = NULL counts the frame's pixels
        pixels = SC.W * SC.H
        frame_rays = np.zeros((pixels + 1, 8), dtype=np.float32); frame_hits = np.zeros((pixels + 1, 8), dtype=np.float32); frame_out = np.zeros((pixels + 1, 16), dtype=np.float32)
        frame_hits.view(np.uint32)[:, 3] = 0xFFFFFFFF
        assert R_.SampleViewRayLights(s.view, frame_rays.ctypes.data, frame_hits.ctypes.data, None, None, None, frame_out.ctypes.data, pixels) == 1, R_.last_error()
        refused("pixels", Sh, lambda: R_.SampleViewRayLights(s.view, frame_rays.ctypes.data, frame_hits.ctypes.data, None, None, None, frame_out.ctypes.data, pixels + 1))
        refused("pixels", St, lambda: R_.TraceViewRaySampledLights(s.view, frame_rays.ctypes.data, None, None, None, None, frame_out.ctypes.data, pixels + 1, 0))
        # J4
        for bad, word in (((17, -1, 0, 0), "maxLights"), ((-2, -1, 0, 0), "maxLights"), ((-1, 65, 0, 0), "diSamples"), ((-1, -2, 0, 0), "diSamples"), ((-1, -1, 1, 0), "sampling flags")):
            p = rt64.LIGHT_SAMPLING(*bad)
            refused(word, Sh, lambda: R_.SampleViewRayLights(s.view, r_, h_, None, k_, C.addressof(p), o_, 4))
            refused(word, Sd, lambda: R_.SampleViewRayLightsDevice(s.view, d_rays, d_hits, None, d_keys, C.addressof(p), d_out, 4, None))
            refused(word, St, lambda: R_.TraceViewRaySampledLights(s.view, r_, None, None, k_, C.addressof(p), o_, 4, 0))
        edge = rt64.LIGHT_SAMPLING(16, 64, 0, 0xFFFFFFFF)                                # the largest accepted values; `reserved` is ignored
        assert R_.SampleViewRayLightsDevice(s.view, d_rays, d_hits, None, d_keys, C.addressof(edge), d_out, 4, None) == 1, R_.last_error()
        assert (out == 0xABABABAB).all()
        m = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], m.vertices, m.indices)
        all_refused("RT64_SetMesh")
        s.draw()
        assert np.array_equal(_bits(rt64.sample_lighting(R_, s.view, rays, hits, None, keys)), _bits(want))          # (explicit keys: the frame count moved, the records did not)
        # the lights are the last drawn frame's
        dark = (rt64.LIGHT * 1)(LC._light(data.lights[0], (0.0, 50.0, 0.0), (0.0, 0.0, 0.0)))
        R_.SetSceneLights(s.scene, dark, 1)
        assert np.array_equal(_bits(rt64.sample_lighting(R_, s.view, rays, hits, None, keys)), _bits(want))
        assert (want[:, 0:3] > 0).any()
        stock = list(data.lights); data.lights = [dark[0]]; s._lights = dark
        s.draw()
        now = rt64.sample_lighting(R_, s.view, rays, hits, None, keys)
        data.lights = stock
        assert not now[:, 0:3].any() and not _bits(now)[:, 7].any() and not _bits(now)[:, 11].any() and np.array_equal(_bits(now)[:, 8:11], _bits(want)[:, 8:11])
        # RT64_DestroyTexture of a texture the frame's table holds (a copy of the floor's diffuse map on an extra instance, which goes first): K9's rule
        t = data.textures[4]
        td = rt64.TEXTURE_DESC(); buf, pitch = t.upload_buffer()
        td.bytes = buf.ctypes.data; td.byteCount = buf.nbytes; td.format = t.format; td.width, td.height, td.rowPitch = t.width, t.height, pitch
        th = R_.CreateTexture(s.device, td)
        assert th, R_.last_error()
        s.textures.append(th)
        ih = R_.CreateInstance(s.scene); s.instances.append(ih)
        floor = data.instances[3]
        s.set_instance(len(s.instances) - 1, sample_scene.InstanceData("extra", floor.mesh, floor.transform, floor.transform, len(s.textures) - 1, None, None, floor.material))
        s.draw()
        assert rt64.sample_lighting(R_, s.view, rays, hits, None, keys) is not None
        R_.DestroyInstance(ih); s.instances.pop()
        R_.DestroyTexture(th); s.textures.pop()
        all_refused("texture")
        s.draw()
        assert np.array_equal(_bits(rt64.sample_lighting(R_, s.view, rays, hits, None, keys)), _bits(now))
    finally:
        hip.close()
        s.close()
