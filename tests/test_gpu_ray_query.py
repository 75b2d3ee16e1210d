"""Ray queries (RT64_TraceViewRays, include/rt64_query.h) against the oracle's traversal, ray by ray and bit for bit (rules Q1-Q7).

The rule is tests/ray_rule.py: oracle/oracle_trace.c's otrace with the closest-hit or accept-first handler, on the TLAS the oracle built for
the same frame.  Seeded rays of the kinds no frame ray reaches -- grazing the floor, starting inside boxes, axis-parallel, zero components,
unnormalised lengths, narrow windows -- on the sample scene (LDS scene cache on and off), on random scenes of tests/test_gpu_fuzz.py
(transformed and mirrored instances, RT64_INSTANCE_DISABLE_BACKFACE_CULLING) and on a sphere of 5120 triangles (multi-kernel builder, HBM
walk with the spill slab).  t, u, v bits, instance and primitive must equal otrace's; with count_traversal = 1 the visit counts too.
"""
import copy

import numpy as np
import pytest

import ray_rule

W, H = 64, 36
FLAG_SETS = (0, ray_rule.CULL_BACK_FACING, ray_rule.ACCEPT_FIRST_HIT, ray_rule.CULL_BACK_FACING | ray_rule.ACCEPT_FIRST_HIT)


def _open(rt64_lib, data, options=None, w=W, h=H):
    from sm64rt_legacy_renderer_amd import sample_scene
    from oracle import oracle_py
    s = sample_scene.Rt64Scene(rt64_lib, data, w, h, hip_device=0)
    for k, v in (options or {}).items():
        assert s.option(k, v), k
    o = oracle_py.OracleScene(data)
    return s, o


def _draw(s, o, w=W, h=H):
    s.draw()
    o.render(w, h, images=False)          # (the oracle's TLAS and instance table of the same frame)


def _same(got, ref, counters=True):
    g, r = got.view(np.uint32), ref.view(np.uint32)
    cols = [0, 1, 2, 3, 4] + ([5, 6] if counters else [])
    bad = np.nonzero((g[:, cols] != r[:, cols]).any(axis=1))[0]
    assert not len(bad), (len(bad), bad[:8].tolist(), got[bad[:3]].tolist(), ref[bad[:3]].tolist())
    if not counters:
        assert not g[:, 5:7].any()        # Q5: only count_traversal = 1 fills them
    assert not g[:, 7].any()


def _query(rt64_lib, s, rays, flags=0):
    from sm64rt_legacy_renderer_amd import rt64
    return rt64.trace_rays(rt64_lib, s.view, rays, flags)


def _check_scene(rt64_lib, data, seed, options, floor=3, flag_sets=FLAG_SETS, n=2000, brute=False):
    s, o = _open(rt64_lib, data, dict(options, count_traversal=1))
    try:
        _draw(s, o)
        rays = ray_rule.random_rays(data, seed, n, floor_instance=floor)
        for flags in flag_sets:
            got, ref = _query(rt64_lib, s, rays, flags), ray_rule.trace(o, rays, flags)
            _same(got, ref)
            assert (got.view(np.int32)[:, 3] >= 0).sum() > n // 20      # the rays do reach geometry
            if flags == 0 and brute:
                # the closest hit does not depend on the walk: the same t as testing every triangle (windows that reach below t = 0 excepted: R2's
                # 1.0000004 widening of tfar narrows a box interval there)
                bf = ray_rule.trace(o, rays, 0, brute_force=True)
                keep = rays[:, 3] >= 0.0
                assert np.array_equal(got[keep, 0].view(np.uint32), bf[keep, 0].view(np.uint32))
        assert s.option("count_traversal", 0)
        _same(_query(rt64_lib, s, rays, 0), ray_rule.trace(o, rays, 0), counters=False)
    finally:
        s.close(); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lds_cache", [1, 0])
def test_sample_scene_rays_match_the_oracle(rt64_lib, sample_data, lds_cache):
    _check_scene(rt64_lib, sample_data, 10 + lds_cache, {"lds_cache": lds_cache}, brute=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 6, 11])
def test_random_scene_rays_match_the_oracle(rt64_lib, sample_data, seed):
    from test_gpu_fuzz import random_scene
    data, _view, _chosen, _per_frame = random_scene(sample_data, seed)
    _check_scene(rt64_lib, data, 100 + seed, {"lds_cache": seed % 2}, flag_sets=(0, ray_rule.CULL_BACK_FACING, ray_rule.ACCEPT_FIRST_HIT), n=1500)


@pytest.mark.gpu
def test_large_mesh_rays_match_the_oracle(rt64_lib):
    """A sphere of 5120 triangles: the multi-kernel BLAS builder, no LDS scene cache, the HBM walk with the query's own spill slab."""
    from sm64rt_legacy_renderer_amd import sample_scene
    data = sample_scene.make_sample_scene(subdiv=2)
    assert len(data.meshes[data.instances[1].mesh].indices) // 3 > 4096
    _check_scene(rt64_lib, data, 7, {}, flag_sets=(0, ray_rule.ACCEPT_FIRST_HIT | ray_rule.CULL_BACK_FACING), n=1500, brute=True)


@pytest.mark.gpu
@pytest.mark.parametrize("lds_cache", [1, 0])
def test_sizes_grid_stride_and_the_end_of_the_array(rt64_lib, sample_data, lds_cache):
    """Counts 1, 63, 64, 65, 255, 256, 257 and RT_GRID_BLOCKS x RT_BLOCK + 65 (the smallest that makes one lane take a second ray of the grid-stride loop),
    closest hit and ACCEPT_FIRST_HIT, walked from the LDS scene cache and from HBM: each equals the prefix of one big call, on the device form (258 guard
    records behind the last one untouched) and, up to 257, on the host form.  Counters included: a ray's record does not depend on its slot or its neighbours."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, sample_data, W, H, hip_device=0)
    hip = ray_rule.Hip()
    try:
        assert s.option("lds_cache", lds_cache) and s.option("count_traversal", 1)
        s.draw()
        rays = ray_rule.random_rays(sample_data, 61 + lds_cache, 2000, floor_instance=3)
        big = 2048 * 256 + 65
        reps = -(-(big + 300) // len(rays))
        rng = np.random.default_rng(5)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(reps - 1)])          # later repetitions shuffled: waves mix instances
        many = np.ascontiguousarray(rays[order])
        n = len(many)
        assert big > 2048 * 256 and n >= big + 258
        d_rays = hip.upload(many)
        guard = np.full((n, 8), 0xABABABAB, dtype=np.uint32)
        for flags in (0, ray_rule.ACCEPT_FIRST_HIT):
            whole = rt64.trace_rays(rt64_lib, s.view, many, flags).view(np.uint32)          # host form: staged in chunks
            first = rt64.trace_rays(rt64_lib, s.view, rays, flags).view(np.uint32)
            assert (first.view(np.int32)[:, 3] >= 0).sum() > len(rays) // 20 and first[:, 5].any()
            assert np.array_equal(whole, first[order]), flags
            for count in (1, 63, 64, 65, 255, 256, 257, big):
                d_guard = hip.upload(guard[:count + 258])
                assert rt64_lib.TraceViewRaysDevice(s.view, d_rays, d_guard, count, flags, None) == 1, rt64_lib.last_error()
                out = hip.download(d_guard, guard[:count + 258])
                assert np.array_equal(out[:count], whole[:count]) and (out[count:] == 0xABABABAB).all(), (flags, count)
                if count <= 257:
                    h_guard = guard[:count + 258].copy()
                    assert rt64_lib.TraceViewRays(s.view, many.ctypes.data, h_guard.ctypes.data, count, flags) == 1
                    assert np.array_equal(h_guard[:count], whole[:count]) and (h_guard[count:] == 0xABABABAB).all(), (flags, count)
    finally:
        hip.close()
        s.close()


@pytest.mark.gpu
def test_camera_ray_picking_agrees_with_the_instance_image(rt64_lib, sample_data):
    from sm64rt_legacy_renderer_amd import rt64
    w, h = 128, 72
    s, o = _open(rt64_lib, sample_data, w=w, h=h)
    try:
        s.draw()
        hit = s.readback(rt64.IMAGE_PRIMARY_HIT)
        inst = np.where(hit[..., 3] == 0xFFFFFFFF, -1, (hit[..., 3] >> 24).astype(np.int64))
        pad = np.pad(inst, 3, mode="edge")
        interior = np.ones_like(inst, dtype=bool)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                interior &= pad[3 + dy:3 + dy + h, 3 + dx:3 + dx + w] == inst
        ys, xs = np.nonzero(interior)
        rng = np.random.default_rng(3)
        pick = rng.choice(len(xs), size=48, replace=False)
        px = np.stack([xs[pick], ys[pick]], axis=1)
        got = _query(rt64_lib, s, ray_rule.camera_rays(sample_data, w, h, px))
        ids = got.view(np.int32)[:, 3]
        assert (ids >= 0).sum() >= 8 and (ids < 0).sum() >= 1         # geometry and sky both picked
        for (x, y), k in zip(px, ids):
            want = rt64_lib.GetViewRaytracedInstanceAt(s.view, int(x), int(y))
            assert rt64_lib.GetViewRaytracedInstance(s.view, int(k)) == want, (x, y, k)
            assert k == inst[y, x]
        assert rt64_lib.GetViewRaytracedInstance(s.view, -1) is None
        assert rt64_lib.GetViewRaytracedInstance(s.view, 1000) is None
    finally:
        s.close(); o.close()


def _moved(inst, dx):
    i = copy.copy(inst)
    t = np.array(inst.transform, dtype=np.float32).copy(); t[3, 0] += np.float32(dx)
    i.transform = t; i.previous_transform = t
    return i


@pytest.mark.gpu
def test_query_on_a_caller_stream_sees_the_frame_it_follows(rt64_lib, sample_data):
    """Enqueued on a caller's stream right after a frame, then the sphere moves and the next frame is drawn at once: the query answers for the
    first frame (its table slot is held until the query has run), a query after the second frame for the second."""
    data = copy.copy(sample_data); data.instances = list(sample_data.instances)
    s, o = _open(rt64_lib, data, {"sync_present": 0})
    hip = ray_rule.Hip()
    try:
        _draw(s, o)
        rays = ray_rule.random_rays(data, 21, 2000, floor_instance=3)
        ref1 = ray_rule.trace(o, rays)
        many = np.ascontiguousarray(np.tile(rays, (64, 1)))
        d_rays, d_hits = hip.upload(many), hip.alloc(many.nbytes)
        st = hip.stream()
        assert rt64_lib.TraceViewRaysDevice(s.view, d_rays, d_hits, len(many), 0, st) == 1, rt64_lib.last_error()
        data.instances[1] = _moved(data.instances[1], 1.5)       # Rt64Scene.draw hands the sphere's description to the library
        o.set_instance(1, data.instances[1])
        s.draw()
        got1 = hip.download(d_hits, many)
        for k in range(0, 64, 9):
            _same(got1[k * len(rays):(k + 1) * len(rays)], ref1, counters=False)
        o.render(W, H, images=False)
        ref2 = ray_rule.trace(o, rays)
        assert not np.array_equal(ref1.view(np.uint32)[:, 0], ref2.view(np.uint32)[:, 0])
        assert rt64_lib.TraceViewRaysDevice(s.view, d_rays, d_hits, len(rays), 0, st) == 1
        _same(hip.download(d_hits, rays), ref2, counters=False)
    finally:
        hip.close()
        s.close(); o.close()


@pytest.mark.gpu
def test_queries_are_refused_when_the_drawn_blas_is_gone(rt64_lib, sample_data):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    data = copy.copy(sample_data); data.instances = list(sample_data.instances)
    s, o = _open(rt64_lib, data)
    rays = ray_rule.random_rays(data, 31, 600, floor_instance=3)
    hits = np.zeros_like(rays)

    def refused():
        ok = rt64_lib.TraceViewRays(s.view, rays.ctypes.data, hits.ctypes.data, len(rays), 0)
        return ok == 0 and len(rt64_lib.last_error()) > 0
    try:
        assert refused()                                             # before the first frame
        assert "draw" in rt64_lib.last_error()
        _draw(s, o)
        _same(_query(rt64_lib, s, rays), ray_rule.trace(o, rays), counters=False)
        # an instance change without a draw: the tables are uploaded at draw time, the answers stay those of the drawn scene
        ref_drawn = ray_rule.trace(o, rays)
        moved = _moved(data.instances[3], 0.75)
        s.set_instance(3, moved)
        _same(_query(rt64_lib, s, rays), ref_drawn, counters=False)
        data.instances[3] = moved; o.set_instance(3, moved)
        _draw(s, o)
        ref_moved = ray_rule.trace(o, rays)
        _same(_query(rt64_lib, s, rays), ref_moved, counters=False)
        # RT64_SetMesh on a mesh the frame traced (same arrays: a rebuild of the same tree, still refused)
        m = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], m.vertices, m.indices)
        assert refused()
        assert "RT64_SetMesh" in rt64_lib.last_error()
        _draw(s, o)
        _same(_query(rt64_lib, s, rays), ref_moved, counters=False)
        # RT64_DestroyMesh on a mesh the frame traced (its instance goes first)
        extra = sample_scene.InstanceData("extra", len(s.meshes), _moved(data.instances[1], -3.0).transform, _moved(data.instances[1], -3.0).transform,
                                          data.instances[1].diffuse, None, None, data.instances[1].material)
        mh = rt64_lib.CreateMesh(s.device, m.flags)
        s.set_mesh(mh, m.vertices, m.indices)
        s.meshes.append(mh)
        ih = rt64_lib.CreateInstance(s.scene)
        s.instances.append(ih)
        s.set_instance(len(s.instances) - 1, extra)
        s.draw()
        assert (_query(rt64_lib, s, rays).view(np.int32)[:, 3] >= 0).any()
        rt64_lib.DestroyInstance(ih); s.instances.pop()
        rt64_lib.DestroyMesh(mh); s.meshes.pop()
        assert refused()
        assert "destroyed" in rt64_lib.last_error()
        _draw(s, o)
        _same(_query(rt64_lib, s, rays), ref_moved, counters=False)
    finally:
        s.close(); o.close()


@pytest.mark.gpu
def test_bad_rays_miss_and_bad_calls_are_refused(rt64_lib, sample_data):
    s, o = _open(rt64_lib, sample_data, {"count_traversal": 1})
    hip = ray_rule.Hip()
    try:
        _draw(s, o)
        good = ray_rule.random_rays(sample_data, 41, 64, floor_instance=3)
        good[:, 7] = np.inf
        bad = []
        nan, inf = np.float32(np.nan), np.float32(np.inf)
        for k in range(8):
            r = good[k % len(good)].copy(); r[k] = nan; bad.append(r)              # a NaN anywhere
        for k in (0, 1, 2, 4, 5, 6):
            for v in (inf, -inf):
                r = good[k].copy(); r[k] = v; bad.append(r)                         # inf in origin or direction
        r = good[3].copy(); r[4:7] = 0.0; bad.append(r)                             # zero direction
        r = good[4].copy(); r[4:7] = -0.0; bad.append(r)
        r = good[5].copy(); r[3] = r[7] = 1.0; bad.append(r)                         # tMin == tMax
        r = good[6].copy(); r[3], r[7] = 2.0, 1.0; bad.append(r)                    # tMin > tMax
        r = good[7].copy(); r[3] = inf; bad.append(r)                               # tMin = +inf = tMax
        bad = np.array(bad, dtype=np.float32)
        assert not any(ray_rule.ray_is_valid(r) for r in bad)
        rays = np.ascontiguousarray(np.concatenate([bad, good]))
        got = _query(rt64_lib, s, rays)
        g = got.view(np.uint32)
        nb = len(bad)
        assert np.all(np.isinf(got[:nb, 0])) and not got[:nb, 1:3].any()
        assert np.all(got.view(np.int32)[:nb, 3] == -1) and np.all(g[:nb, 4] == 0xFFFFFFFF) and not g[:nb, 5:8].any()
        _same(got[nb:], ray_rule.trace(o, good))                                   # tMax = +inf rays hit as usual
        assert (got.view(np.int32)[nb:, 3] >= 0).any()
        # count = 0 succeeds; NULL arrays, a NULL view, unknown flags and unaligned device arrays are refused
        hits = np.zeros_like(rays)
        assert rt64_lib.TraceViewRays(s.view, rays.ctypes.data, hits.ctypes.data, 0, 0) == 1
        assert rt64_lib.TraceViewRays(s.view, None, hits.ctypes.data, 4, 0) == 0 and rt64_lib.last_error()
        assert rt64_lib.TraceViewRays(s.view, rays.ctypes.data, None, 4, 0) == 0
        assert rt64_lib.TraceViewRays(None, rays.ctypes.data, hits.ctypes.data, 4, 0) == 0
        assert rt64_lib.TraceViewRays(s.view, rays.ctypes.data, hits.ctypes.data, 4, 0x100) == 0
        d_rays, d_hits = hip.upload(rays), hip.alloc(rays.nbytes)
        assert rt64_lib.TraceViewRaysDevice(s.view, None, d_hits, 4, 0, None) == 0
        assert rt64_lib.TraceViewRaysDevice(s.view, d_rays + 4, d_hits, 4, 0, None) == 0
        assert "aligned" in rt64_lib.last_error()
        # the device form on the device's stream (stream = NULL) returns after completion
        assert rt64_lib.TraceViewRaysDevice(s.view, d_rays, d_hits, len(rays), 0, None) == 1
        assert np.array_equal(hip.download(d_hits, rays).view(np.uint32), g)
    finally:
        hip.close()
        s.close(); o.close()


@pytest.mark.gpu
def test_queries_between_frames_leave_the_frames_alone(rt64_lib, sample_data):
    """A C3-style sequence (GI + SVGF history, the camera drifting) with queries between its frames -- host arrays, and device arrays on a caller
    stream -- renders byte-identical images to the same sequence without them."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    rays = ray_rule.random_rays(sample_data, 51, 4000, floor_instance=3)
    images = (rt64.IMAGE_FINAL_RGBA8, rt64.IMAGE_OUTPUT_RGBA32F, rt64.IMAGE_INDIRECT_LIGHT_FILTERED, rt64.IMAGE_PRIMARY_HIT)

    def run(query):
        data = copy.copy(sample_data)
        s = sample_scene.Rt64Scene(rt64_lib, data, 96, 64, hip_device=0)
        hip = ray_rule.Hip()
        try:
            s.set_view_description(gi_samples=1, denoiser=True)
            assert s.option("denoiser_mode", 1)
            out = []
            st = hip.stream()
            d_rays, d_hits = hip.upload(rays), hip.alloc(rays.nbytes)
            for f in range(4):
                v = np.array(sample_data.view, dtype=np.float32).copy(); v[3, 0] += np.float32(0.05 * f)
                data.view = v
                s.draw()
                if query:
                    rt64.trace_rays(rt64_lib, s.view, rays, rt64.RAY_FLAG_CULL_BACK_FACING)
                    assert rt64_lib.TraceViewRaysDevice(s.view, d_rays, d_hits, len(rays), rt64.RAY_FLAG_ACCEPT_FIRST_HIT, st) == 1
                out.append([s.readback(k).copy() for k in images])
            return out
        finally:
            hip.close()
            s.close()
    a, b = run(False), run(True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert x.tobytes() == y.tobytes()
