"""Layered ray queries (RT64_TraceViewRayLayers, RT64_WeighViewRayLayers, include/rt64_layers.h) on the GPU, held to the float64 rule of tests/layers_rule.py ray by
ray (rules T1-T12), to the closest-hit walk (T9), to a frame's own images (T10) and to themselves: the forms agree byte for byte, with and without the
LDS scene cache, the composite call is the two steps, nothing is written past the last record and every slot before it is, bad calls are refused as T11 says, and
frames do not notice.

The candidates of every ray come from the oracle's enumeration (tests/alpha_rule.py), their alphas from tests/material_rule.py, the lists of class (c) from the
oracle's ordered walk.  One run's lines of the first test are committed as profiles/layers_rule_deviation.txt.
"""
import copy

import numpy as np
import pytest

import layers_cases as LC
import layers_rule as R
import material_cases as MC
import material_rule as M
import ray_rule
from test_layers_rule import MUTATION_CASES, SEEDS

pytestmark = pytest.mark.gpu

W, H = LC.W, LC.H
CULL = ray_rule.CULL_BACK_FACING
L16 = R.LAYERS_MAX
GUARD = 0xABABABAB


def _open(rt64_lib, data, options=None, w=W, h=H):
    from sm64rt_legacy_renderer_amd import sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, data, w, h, hip_device=0)
    for k, v in (options or {}).items():
        assert s.option(k, v), k
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rule(data, rays, cull=False, mutate=None):
    o, cand = LC.enumerate_candidates(data, rays, cull)
    try:
        return R.lists(data, M.texture_levels(data), rays, cand, cull=cull, oracle_scene=o, mutate=mutate)
    finally:
        o.close()


@pytest.mark.parametrize("name", LC.NAMES)
def test_the_lists_and_weights_lie_within_the_rule_ray_by_ray(rt64_lib, oracle_lib, sample_data, name):
    """1.  Per case: count, flags, instance and primitive exact and t, u, v bit-equal on every decided ray, class (c) included (the oracle's ordered walk); weights,
    transmittance and refraction within the derived bound, shaded and the coverage flags exact.  The mutations assigned to the case leave the device's results."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K, classes = LC.case(sample_data, name)
    rays = LC.rays_of(K, SEEDS[name])
    s = _open(rt64_lib, data)
    try:
        s.draw()
        hits, layers, weights, coverage = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, L16, weights=True)
    finally:
        s.close()
    rule = _rule(data, rays)
    wrule = R.weights(rule)
    c = R.compare(rule, wrule, hits, layers, weights, coverage)
    cls = np.array(rule["cls"]); length = np.array([len(r) for r in rule["rows"]])
    decided = ~wrule["undecided"]
    print("%-16s rays %3d  classes a/b/c %3d/%3d/%3d (decided, two or more layers)  longest list %2d  ends opaque %3d  full %3d  undecided %.4f  lists that differ %d  "
          "largest weight ratio %.3f  largest bound %.2e  coverage records that differ %d  covered %3d  glass %3d" %
          (name, len(rays), *[int(((cls == x) & decided & (length >= 2)).sum()) for x in "abc"], int(length.max()), int(rule["ends_opaque"].sum()), int(rule["full"].sum()),
           wrule["undecided"].mean(), int((~c["lists"]).sum()), c["ratio"].max(), wrule["e"].max(), int((~c["coverage"]).sum()),
           int(((wrule["flags"] & R.COVERAGE_COVERED) != 0).sum()), int(((wrule["flags"] & R.COVERAGE_GLASS) != 0).sum())))
    assert wrule["undecided"].mean() <= 0.02
    for x in classes:
        assert ((cls == x) & decided & (length >= 2)).sum() >= 32, (name, x)
    assert c["lists"].all(), (name, np.nonzero(~c["lists"])[0][:8].tolist())
    assert (c["ratio"] <= 1.0).all(), (name, float(c["ratio"].max()), np.nonzero(~(c["ratio"] <= 1.0))[0][:8].tolist())
    assert c["coverage"].all(), (name, np.nonzero(~c["coverage"])[0][:8].tolist())
    assert not _bits(hits)[:, :, 5:8].any()                                                      # T6: a layer's own counters are 0
    for mutation, where in MUTATION_CASES.items():
        if where != name or mutation == "covered_never_stops":
            continue
        mrule = _rule(data, rays, mutate=mutation)
        m = R.compare(mrule, R.weights(mrule, mutate=mutation), hits, layers, weights, coverage)
        out = ~m["lists"] | ~(m["ratio"] <= 1.0) | ~m["coverage"]
        print("    mutation %-28s %4d of %4d of the device's rays outside it" % (mutation, int(out.sum()), len(out)))
        assert out.sum() >= 1, mutation


def test_a_bad_record_behind_complete_coverage_is_not_read(rt64_lib, sample_data):
    """T7: the resolve stops at complete coverage -- a record with an out-of-range instance behind it does not set BAD_HIT, one in front of it does (what the mutation
    covered_never_stops gets wrong); an out-of-range primitive counts as well."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K, _ = LC.case(sample_data, "instances_3")
    rays = LC.rays_of(K, SEEDS["instances_3"])
    s = _open(rt64_lib, data)
    try:
        s.draw()
        hits, layers = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 8)
        count = layers[:, 0].astype(np.int64)
        bad = hits.copy(); bb = _bits(bad)
        for k in range(len(rays)):
            bb[count[k], k, 3] = 1000 + k; bb[count[k], k, 4] = 0
        weights, coverage = rt64.weigh_view_ray_layers(rt64_lib, s.view, rays, bad)
        w0, c0 = rt64.weigh_view_ray_layers(rt64_lib, s.view, rays, hits)
        flags, f0 = _bits(coverage)[:, 3], _bits(c0)[:, 3]
        valid = (f0 & R.COVERAGE_VALID) != 0
        covered = (f0 & R.COVERAGE_COVERED) != 0
        assert covered.sum() >= 32 and (valid & ~covered).sum() >= 32
        assert np.array_equal(flags[covered], f0[covered]) and np.array_equal(flags[valid & ~covered], f0[valid & ~covered] | R.COVERAGE_BAD_HIT)
        assert np.array_equal(_bits(weights), _bits(w0)) and np.array_equal(_bits(coverage)[:, :3], _bits(c0)[:, :3])
        bb[:, :, 3] = _bits(hits)[:, :, 3]
        open_ = valid & (count > 0)
        bb[0, :, 4] = 0x00FFFFFF                                                               # an out-of-range primitive in layer 0
        _, coverage = rt64.weigh_view_ray_layers(rt64_lib, s.view, rays, bad)
        assert ((_bits(coverage)[open_, 3] & R.COVERAGE_BAD_HIT) != 0).all() and (coverage[open_, 0] == 1.0).all()
    finally:
        s.close()


def test_the_equivalences_hold_on_the_device(rt64_lib, sample_data):
    """2.  T9: on the sample scene (every instance O1-opaque, depthBias 0) layer 0 at maxLayers = 1 is RT64_TraceViewRaysAlpha's t, u, v, instance, primitive byte for
    byte, under both flags; and the output for maxLayers = 1, 2, 5 is the prefix of the output for 16, on the sample scene and on a stack."""
    from sm64rt_legacy_renderer_amd import rt64
    data = MC.small_sample(sample_data)
    rays = ray_rule.random_rays(data, 301, 2000, floor_instance=3)
    s = _open(rt64_lib, data)
    try:
        s.draw()
        for flags in (0, CULL):
            one, lay = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 1, flags=flags)
            plain = rt64.trace_rays_alpha(rt64_lib, s.view, rays, None, flags)
            assert np.array_equal(_bits(one)[0, :, :5], _bits(plain)[:, :5])
            hit = _bits(plain)[:, 3] != 0xFFFFFFFF
            assert hit.sum() > 100 and np.array_equal(lay[:, 0], hit.astype(np.uint32)) and (lay[hit, 1] == (R.LAYERS_VALID | R.LAYERS_ENDS_OPAQUE)).all()
    finally:
        s.close()
    for data, rays in ((data, rays), (LC.case(sample_data, "depth_bias_20")[0], LC.rays_of(20, 7))):
        s = _open(rt64_lib, data)
        try:
            s.draw()
            full, lay = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, L16)
            for m in (1, 2, 5, 16):
                part, play = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, m)
                assert np.array_equal(_bits(part), _bits(full)[:m])
                assert np.array_equal(play[:, 0], np.minimum(lay[:, 0], m)) and np.array_equal(play[:, 1:], lay[:, 1:])
        finally:
            s.close()


@pytest.mark.parametrize("name", ["instances_8", "depth_bias_20"])
def test_camera_rays_agree_with_the_frame(rt64_lib, sample_data, name):
    """3.  T10 at 64 x 36, every G-buffer image written: layer 0 of a pixel's camera ray is RT64_IMAGE_PRIMARY_HIT's t, u, v bits, instance and primitive; 1 -
    transmittance is the alpha of RT64_IMAGE_DIFFUSE within 1 / 255 plus the weight bound, on the pixels whose list is not FULL."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K, _ = LC.case(sample_data, name)
    s = _open(rt64_lib, data, {"lean_frames": 0})
    try:
        s.draw()
        shown = s.readback(rt64.IMAGE_PRIMARY_HIT).reshape(-1, 4)
        diffuse = s.readback(rt64.IMAGE_DIFFUSE).reshape(-1, 4)
        rays = rt64.camera_rays(rt64_lib, s.view, count=W * H, differentials=False)
        hits, layers, weights, coverage = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, L16, flags=CULL, weights=True)
    finally:
        s.close()
    first = _bits(hits)[0]
    hit = shown[:, 3] != 0xFFFFFFFF
    assert hit.sum() > 500 and np.array_equal(hit, layers[:, 0] > 0)
    assert np.array_equal(first[hit, :3], shown[hit, :3])
    assert np.array_equal(first[hit, 3], shown[hit, 3] >> 24) and np.array_equal(first[hit, 4] & 0xFFFFFF, shown[hit, 3] & 0xFFFFFF)
    open_ = (layers[:, 1] & R.LAYERS_FULL) == 0
    bound = 1.0 / 255.0 + (2 * L16 + 2) * 2.0 ** -24
    alpha = 1.0 - coverage[:, 0].astype(np.float64)
    assert (open_ & (layers[:, 0] >= 2)).sum() >= 32
    assert (np.abs(alpha - diffuse[:, 3])[open_] <= bound).all(), float(np.abs(alpha - diffuse[:, 3])[open_].max())


def test_the_forms_agree_byte_for_byte(rt64_lib, sample_data):
    """4.  Host arrays, device arrays on the device's stream and on a caller stream give the same records; lods = NULL is an array of zeros; lds_cache 0 and 1 agree;
    the composite call is the two steps (T8)."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K, _ = LC.case(sample_data, "ignored_hits_20")
    rays = LC.rays_of(K, 11)
    results = []
    for cache in (1, 0):
        s = _open(rt64_lib, data, {"lds_cache": cache})
        hip = ray_rule.Hip()
        try:
            s.draw()
            n = len(rays)
            d_rays, d_lods = hip.upload(rays), hip.upload(np.zeros(n, dtype=np.float32))
            for m in (16, 3):
                hits, layers, weights, coverage = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, m, weights=True)
                h2, l2 = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, m)
                w2, c2 = rt64.weigh_view_ray_layers(rt64_lib, s.view, rays, h2)
                for x, y in ((hits, h2), (layers, l2), (weights, w2), (coverage, c2)):
                    assert np.array_equal(_bits(x), _bits(y))                                   # T8
                assert (layers[:, 0] >= 2).sum() > 100 and (weights > 0).sum() > 200
                results.append((hits, layers, weights, coverage))
                for st, l in ((None, None), (hip.stream(), d_lods)):
                    d_hits, d_layers, d_w, d_c = hip.alloc(hits.nbytes), hip.alloc(layers.nbytes), hip.alloc(weights.nbytes), hip.alloc(coverage.nbytes)
                    assert rt64_lib.TraceViewRayLayersDevice(s.view, d_rays, l, m, d_hits, d_layers, n, 0, st) == 1, rt64_lib.last_error()
                    assert rt64_lib.WeighViewRayLayersDevice(s.view, d_rays, d_hits, l, m, d_w, d_c, n, st) == 1, rt64_lib.last_error()
                    if st:
                        assert hip.h.hipStreamSynchronize(st) == 0
                    for d, like in ((d_hits, hits), (d_layers, layers), (d_w, weights), (d_c, coverage)):
                        assert np.array_equal(_bits(hip.download(d, like)), _bits(like))
        finally:
            hip.close()
            s.close()
    for a, b in zip(results[:2], results[2:]):
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))                                           # lds_cache 1 against 0


def test_sizes_grid_stride_and_the_ends_of_the_arrays(rt64_lib, sample_data):
    """5.  Counts 1, 63, 64, 65, 255, 256, 257 and RT_GRID_BLOCKS x RT_BLOCK + 1 at maxLayers = 2: each equals the rays' own records whatever their place, every slot
    of the four arrays is written and the guard words behind each are untouched, on the device forms and (the small counts) the host form."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K, _ = LC.case(sample_data, "instances_8")
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = LC.rays_of(K, 29)
        big, m = 2048 * 256 + 1, 2
        reps = -(-big // len(rays))
        rng = np.random.default_rng(5)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(reps - 1)])[:big]
        many = np.ascontiguousarray(rays[order])
        fh, fl, fw, fc = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, m, weights=True)
        d_rays = hip.upload(many)
        for count in (1, 63, 64, 65, 255, 256, 257, big):
            want = (_bits(fh)[:, order[:count]], _bits(fl)[order[:count]], _bits(fw)[:, order[:count]], _bits(fc)[order[:count]])
            shapes = [(m * count + 7, 8), (count + 7, 4), (m * count + 7,), (count + 7, 4)]
            bufs = [hip.upload(np.full(sh, GUARD, dtype=np.uint32)) for sh in shapes]
            assert rt64_lib.TraceViewRayLayersDevice(s.view, d_rays, None, m, bufs[0], bufs[1], count, 0, None) == 1, rt64_lib.last_error()
            assert rt64_lib.WeighViewRayLayersDevice(s.view, d_rays, bufs[0], None, m, bufs[2], bufs[3], count, None) == 1, rt64_lib.last_error()
            for b, sh, w in zip(bufs, shapes, want):
                out = hip.download(b, np.empty(sh, dtype=np.uint32))
                used = w.size // (sh[1] if len(sh) == 2 else 1)
                assert np.array_equal(out[:used].reshape(w.shape), w) and (out[used:] == GUARD).all(), (count, sh)
            if count <= 257:
                host = [np.full(sh, GUARD, dtype=np.uint32) for sh in shapes]
                assert rt64_lib.TraceViewRayLayers(s.view, many.ctypes.data, None, m, host[0].ctypes.data, host[1].ctypes.data, host[2].ctypes.data, host[3].ctypes.data, count, 0) == 1
                for out, sh, w in zip(host, shapes, want):
                    used = w.size // (sh[1] if len(sh) == 2 else 1)
                    assert np.array_equal(out[:used].reshape(w.shape), w) and (out[used:] == GUARD).all(), (count, sh)
            for b in bufs:
                assert hip.h.hipFree(b) == 0
                hip.ptrs.remove(b)
    finally:
        hip.close()
        s.close()


@pytest.mark.parametrize("m, count", [(16, 16384 + 65), (3, 87381 + 1)])
def test_host_arrays_that_cross_a_chunk_agree_with_the_device_form(rt64_lib, sample_data, m, count):
    """5b.  The host forms stage 2^18 / maxLayers rays per round trip: 16384 at 16 layers, 87381 (no power of two) at 3.  One ray more than a chunk (65 more at 16
    layers): RT64_TraceViewRayLayers with weights and coverage, and RT64_WeighViewRayLayers fed with the device walk's hits (the layer-major gather on the way up),
    equal the device forms -- which do not chunk -- bit for bit on the same rays, and the spare records behind each host array keep their guard words."""
    data, K, _ = LC.case(sample_data, "instances_8")
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = LC.rays_of(K, 29)
        rng = np.random.default_rng(7)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(-(-count // len(rays)) - 1)])[:count]
        many = np.ascontiguousarray(rays[order])
        shapes = [(m * count, 8), (count, 4), (m * count,), (count, 4)]
        d_rays = hip.upload(many)
        bufs = [hip.alloc(4 * int(np.prod(sh))) for sh in shapes]
        assert rt64_lib.TraceViewRayLayersDevice(s.view, d_rays, None, m, bufs[0], bufs[1], count, 0, None) == 1, rt64_lib.last_error()
        assert rt64_lib.WeighViewRayLayersDevice(s.view, d_rays, bufs[0], None, m, bufs[2], bufs[3], count, None) == 1, rt64_lib.last_error()
        want = [hip.download(b, np.empty(sh, dtype=np.uint32)) for b, sh in zip(bufs, shapes)]
        assert (want[1][:, 0] >= 2).sum() >= 32 and len(np.unique(want[2])) > 2          # lists with layers behind the first, weights that differ
        spare = [(sh[0] + 7,) + sh[1:] for sh in shapes]
        host = [np.full(sh, GUARD, dtype=np.uint32) for sh in spare]
        assert rt64_lib.TraceViewRayLayers(s.view, many.ctypes.data, None, m, host[0].ctypes.data, host[1].ctypes.data, host[2].ctypes.data, host[3].ctypes.data, count, 0) == 1, rt64_lib.last_error()
        for out, w in zip(host, want):
            assert np.array_equal(out[:len(w)], w) and (out[len(w):] == GUARD).all(), (m, w.shape)
        weighed = [np.full(sh, GUARD, dtype=np.uint32) for sh in spare[2:]]
        assert rt64_lib.WeighViewRayLayers(s.view, many.ctypes.data, want[0].ctypes.data, None, m, weighed[0].ctypes.data, weighed[1].ctypes.data, count) == 1, rt64_lib.last_error()
        for out, w in zip(weighed, want[2:]):
            assert np.array_equal(out[:len(w)], w) and (out[len(w):] == GUARD).all(), (m, w.shape)
    finally:
        hip.close()
        s.close()


def test_counters_follow_count_traversal(rt64_lib, sample_data):
    """6.  T6: RT64_RAY_LAYERS' counters are 0 without count_traversal; with it non-zero for the rays that were walked into the scene and 0 for Q6-invalid rays; the
    layers' own counters stay 0."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K, _ = LC.case(sample_data, "instances_8")
    rays = LC.rays_of(K, 33)
    s = _open(rt64_lib, data)
    try:
        s.draw()
        hits, layers = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 4)
        assert not layers[:, 2:].any() and not _bits(hits)[:, :, 5:8].any()
        assert s.option("count_traversal", 1)
        s.draw()
        h2, l2 = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 4)
        assert np.array_equal(_bits(h2), _bits(hits)) and np.array_equal(l2[:, :2], layers[:, :2])
        hit = l2[:, 0] > 0
        assert hit.sum() > 100 and (l2[hit, 2] > 0).all() and (l2[hit, 3] > 0).all()
        invalid = l2[:, 1] == 0
        assert invalid.sum() >= 8 and not l2[invalid].any()
    finally:
        s.close()


def test_refusals(rt64_lib, sample_data):
    """7.  T11, one by one: every refusal returns 0 with a message that names the function; count = 0 succeeds and touches nothing; a destroyed texture refuses the
    calls until the next frame."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    data = MC.small_sample(sample_data)
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    R_ = rt64_lib
    try:
        rays = ray_rule.random_rays(data, 31, 600, floor_instance=3)
        n, m = len(rays), 2
        hits = np.full((m, n, 8), GUARD, dtype=np.uint32); lay = np.full((n, 4), GUARD, dtype=np.uint32)
        wts = np.full((m, n), GUARD, dtype=np.uint32); cov = np.full((n, 4), GUARD, dtype=np.uint32)
        T, TD, G, GD = "RT64_TraceViewRayLayers", "RT64_TraceViewRayLayersDevice", "RT64_WeighViewRayLayers", "RT64_WeighViewRayLayersDevice"
        d_rays, d_hits, d_lay, d_w, d_cov = hip.upload(rays), hip.upload(hits), hip.alloc(lay.nbytes), hip.alloc(wts.nbytes), hip.alloc(cov.nbytes)
        d_lods = hip.upload(np.zeros(n, dtype=np.float32))
        rp, hp, lp, wp, cp = rays.ctypes.data, hits.ctypes.data, lay.ctypes.data, wts.ctypes.data, cov.ctypes.data

        def refused(word, fn, call):
            ok = call()
            assert ok == 0 and fn + ":" in R_.last_error() and word in R_.last_error(), (ok, R_.last_error())

        def all_refused(word):
            refused(word, T, lambda: R_.TraceViewRayLayers(s.view, rp, None, m, hp, lp, wp, cp, n, 0))
            refused(word, TD, lambda: R_.TraceViewRayLayersDevice(s.view, d_rays, None, m, d_hits, d_lay, 4, 0, None))
            refused(word, G, lambda: R_.WeighViewRayLayers(s.view, rp, hp, None, m, wp, cp, n))
            refused(word, GD, lambda: R_.WeighViewRayLayersDevice(s.view, d_rays, d_hits, None, m, d_w, d_cov, 4, None))
        all_refused("draw")                                                               # before the first frame
        s.draw()
        assert R_.TraceViewRayLayers(s.view, rp, None, m, hp, lp, wp, cp, 0, 0) == 1 and R_.WeighViewRayLayers(s.view, rp, hp, None, m, wp, cp, 0) == 1
        assert R_.TraceViewRayLayersDevice(s.view, d_rays, None, m, d_hits, d_lay, 0, 0, None) == 1 and R_.WeighViewRayLayersDevice(s.view, d_rays, d_hits, None, m, d_w, d_cov, 0, None) == 1
        for bad in (0, 17, 0xFFFFFFFF):
            refused("maxLayers", T, lambda: R_.TraceViewRayLayers(s.view, rp, None, bad, hp, lp, wp, cp, 4, 0))
            refused("maxLayers", TD, lambda: R_.TraceViewRayLayersDevice(s.view, d_rays, None, bad, d_hits, d_lay, 4, 0, None))
            refused("maxLayers", G, lambda: R_.WeighViewRayLayers(s.view, rp, hp, None, bad, wp, cp, 4))
            refused("maxLayers", GD, lambda: R_.WeighViewRayLayersDevice(s.view, d_rays, d_hits, None, bad, d_w, d_cov, 4, None))
        for flags in (0x2, 0x4, 0x80000000):
            refused("unknown flags", T, lambda: R_.TraceViewRayLayers(s.view, rp, None, m, hp, lp, None, None, 4, flags))
            refused("unknown flags", TD, lambda: R_.TraceViewRayLayersDevice(s.view, d_rays, None, m, d_hits, d_lay, 4, flags, None))
        refused("NULL", T, lambda: R_.TraceViewRayLayers(s.view, None, None, m, hp, lp, None, None, 4, 0))
        refused("NULL", T, lambda: R_.TraceViewRayLayers(s.view, rp, None, m, None, lp, None, None, 4, 0))
        refused("NULL", T, lambda: R_.TraceViewRayLayers(s.view, rp, None, m, hp, None, None, None, 4, 0))
        refused("NULL view", T, lambda: R_.TraceViewRayLayers(None, rp, None, m, hp, lp, None, None, 4, 0))
        refused("NULL", TD, lambda: R_.TraceViewRayLayersDevice(s.view, d_rays, None, m, None, d_lay, 4, 0, None))
        refused("NULL", G, lambda: R_.WeighViewRayLayers(s.view, rp, hp, None, m, None, cp, 4))
        refused("NULL", G, lambda: R_.WeighViewRayLayers(s.view, rp, hp, None, m, wp, None, 4))
        refused("NULL", G, lambda: R_.WeighViewRayLayers(s.view, rp, None, None, m, wp, cp, 4))
        refused("NULL", GD, lambda: R_.WeighViewRayLayersDevice(s.view, d_rays, d_hits, None, m, None, d_cov, 4, None))
        refused("NULL view", GD, lambda: R_.WeighViewRayLayersDevice(None, d_rays, d_hits, None, m, d_w, d_cov, 4, None))
        for a, l, b, c in ((d_rays + 4, None, d_hits, d_lay), (d_rays, None, d_hits + 8, d_lay), (d_rays, None, d_hits, d_lay + 4), (d_rays, d_lods + 2, d_hits, d_lay)):
            refused("aligned", TD, lambda: R_.TraceViewRayLayersDevice(s.view, a, l, m, b, c, 4, 0, None))
        for a, b, w, c in ((d_rays + 8, d_hits, d_w, d_cov), (d_rays, d_hits + 4, d_w, d_cov), (d_rays, d_hits, d_w + 2, d_cov), (d_rays, d_hits, d_w, d_cov + 8)):
            refused("aligned", GD, lambda: R_.WeighViewRayLayersDevice(s.view, a, b, None, m, w, c, 4, None))
        assert (hits == GUARD).all() and (lay == GUARD).all() and (wts == GUARD).all() and (cov == GUARD).all()
        assert R_.TraceViewRayLayersDevice(s.view, d_rays, d_lods + 4, m, d_hits, d_lay, 4, 0, None) == 1          # lods need 4-byte alignment only
        assert R_.WeighViewRayLayersDevice(s.view, d_rays, d_hits, None, m, d_w + 4, d_cov, 4, None) == 1          # and so do weights
        want = rt64.trace_view_ray_layers(R_, s.view, rays, m, weights=True)
        # RT64_SetMesh on a mesh the frame traced: refused until the next frame
        msh = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], msh.vertices, msh.indices)
        all_refused("RT64_SetMesh")
        s.draw()
        # RT64_DestroyTexture of a texture the frame's table holds (a copy of the floor's diffuse map on an extra instance, which goes first)
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
        assert rt64.trace_view_ray_layers(R_, s.view, rays, m, weights=True) is not None
        R_.DestroyInstance(ih); s.instances.pop()
        R_.DestroyTexture(th); s.textures.pop()
        all_refused("texture")
        s.draw()
        got = rt64.trace_view_ray_layers(R_, s.view, rays, m, weights=True)
        for x, y in zip(got, want):
            assert np.array_equal(_bits(x), _bits(y))
    finally:
        hip.close()
        s.close()


def test_a_walk_on_a_caller_stream_outlives_its_texture(rt64_lib, sample_data):
    """8.  K9's texture lifetime: enqueued on a caller's stream, followed at once by RT64_DestroyTexture of a texture the walk reads (the edge sheet's) and by a new
    frame: the records are the bytes of the synchronous call made before it."""
    from sm64rt_legacy_renderer_amd import rt64
    data, K, _ = LC.case(sample_data, "ignored_hits_8")
    rays = LC.rays_of(K, 21)
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
        first, lay = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 4)
        reps = 64
        many = np.ascontiguousarray(np.tile(rays, (reps, 1)))
        like_h, like_l = np.empty((4, len(many), 8), dtype=np.float32), np.empty((len(many), 4), dtype=np.uint32)
        d_rays, d_hits, d_lay = hip.upload(many), hip.alloc(like_h.nbytes), hip.alloc(like_l.nbytes)
        st = hip.stream()
        assert rt64_lib.TraceViewRayLayersDevice(s.view, d_rays, None, 4, d_hits, d_lay, len(many), 0, st) == 1, rt64_lib.last_error()
        s.set_instance(edge, data.instances[edge])
        rt64_lib.DestroyTexture(th); s.textures.pop()
        s.draw()
        got = _bits(hip.download(d_hits, like_h)).reshape(4, reps, len(rays), 8)
        assert (got == _bits(first)[:, None]).all()
        assert (hip.download(d_lay, like_l).reshape(reps, len(rays), 4) == lay[None]).all()
    finally:
        hip.close()
        s.close()


@pytest.mark.parametrize("streams", [1, 3])
def test_layer_queries_between_frames_leave_the_frames_alone(rt64_lib, sample_data, streams, monkeypatch):
    """9.  A GI + denoiser sequence with layer queries between its frames -- host arrays, and device arrays on a caller stream -- renders byte-identical images to the
    same sequence without them, on one render stream and on three."""
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
            d_rays, d_hits, d_lay, d_w, d_cov = hip.upload(rays), hip.alloc(3 * n * 32), hip.alloc(n * 16), hip.alloc(3 * n * 4), hip.alloc(n * 16)
            for f in range(3):
                v = np.array(sample_data.view, dtype=np.float32).copy(); v[3, 0] += np.float32(0.05 * f)
                data.view = v
                s.draw()
                hits = rt64.trace_rays(rt64_lib, s.view, rays)
                if query:
                    rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 16, flags=CULL, weights=True)
                    assert rt64_lib.TraceViewRayLayersDevice(s.view, d_rays, None, 3, d_hits, d_lay, n, 0, st) == 1
                    assert rt64_lib.WeighViewRayLayersDevice(s.view, d_rays, d_hits, None, 3, d_w, d_cov, n, st) == 1
                out.append([s.readback(k).copy() for k in images] + [hits])
            return out
        finally:
            hip.close()
            s.close()
    a, b = run(False), run(True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert x.tobytes() == y.tobytes()
