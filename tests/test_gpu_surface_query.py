"""Surface records of ray-query hits (RT64_ResolveViewRayHits, include/rt64_surface.h) on the GPU, held to the float64 rule of tests/surface_rule.py hit by hit
(rules A1-A9), to the frame's own G-buffer, and to themselves: the three forms agree byte for byte, the grid-stride loop repeats itself exactly,
nothing is written past the last record, bad hits and bad calls are answered as A2 / A3 / A9 say, and frames do not notice.

The hits come from the library's own walk (rt64.trace_rays; tests/test_gpu_ray_query.py holds that to the oracle bit for bit).  One run's lines of the first test
are committed as profiles/surface_rule_deviation.txt.
"""
import copy

import numpy as np
import pytest

import ray_rule
import surface_cases
import surface_rule as S

pytestmark = pytest.mark.gpu

W, H = 64, 36
REC = 64          # bytes of an RT64_RAY_SURFACE


def _open(rt64_lib, data, options=None, w=W, h=H):
    from sm64rt_legacy_renderer_amd import sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, data, w, h, hip_device=0)
    for k, v in (options or {}).items():
        assert s.option(k, v), k
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _held_to_the_rule(name, data, rays, hits, got, say=True):
    rule = S.surfaces(data, rays, hits)
    ratios, exact = S.compare(rule, got)
    if say:
        print(S.report(name, rule, ratios, exact))
    real = rule["kind"] == 2
    assert exact.all(), (name, np.nonzero(~exact)[0][:8].tolist())
    for k, r in ratios.items():
        assert (r < 1.0).all(), (name, k, float(r.max()), np.nonzero(~(r < 1.0))[0][:8].tolist())
    return rule, real


CASES = ["sample lds_cache=1", "sample lds_cache=0", "sphere 5120 triangles", "random scene 3", "random scene 6", "rotation x scale (1, .5, 2)", "mirrored x = -1",
         "zero vertex normals", "no UV layout"]


@pytest.fixture(scope="module")
def cases(sample_data):
    return {name: (data, seed, options) for name, data, seed, options in surface_cases.cases(sample_data)}


@pytest.mark.parametrize("name", CASES)
def test_records_lie_within_the_rule_hit_by_hit(rt64_lib, cases, name):
    """1.  |record - rule| / bound < 1 for position, both normals and uv; integers, flags and t exact; the bound itself is not vacuous; few hits undecided."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options = cases[name]
    s = _open(rt64_lib, data, options)
    try:
        s.draw()
        rays = ray_rule.random_rays(data, seed, surface_cases.RAYS, floor_instance=3)
        hits = rt64.trace_rays(rt64_lib, s.view, rays)
        got = rt64.resolve_hits(rt64_lib, s.view, rays, hits)
    finally:
        s.close()
    rule, real = _held_to_the_rule(name, data, rays, hits, got)
    assert real.sum() > surface_cases.RAYS // 20 and np.array_equal(real, hits.view(np.int32)[:, 3] >= 0)
    lo, hi = ray_rule.scene_bounds(data)
    assert rule["position"][1][real].max() <= 1e-4 * float((hi - lo).max())
    assert max(rule["geometric"][1][real].max(), rule["shading"][1][real].max()) <= 1e-4
    assert rule["has_uv"][real].all() == (name != "no UV layout") and rule["has_uv"][real].any() == (name != "no UV layout")
    if name != "no UV layout":
        assert rule["uv"][1][real].max() <= 1e-4 * np.abs(rule["uv"][0][real]).max()
    assert rule["undecided"][real].mean() <= 0.01
    if name == "zero vertex normals":          # A7's fallback: on the sphere the shading normal is the geometric normal, flipped towards the ray
        sph = real & (rule["instance"] == 0)
        sign = np.where(_bits(got)[sph, 3] & S.BACK_FACE, -1.0, 1.0)[:, None]
        assert np.abs(got[sph, 8:11] - got[sph, 4:7] * sign).max() < 1e-5


def test_records_agree_with_the_frame(rt64_lib, sample_data):
    """2.  Camera rays of pixels well inside one opaque instance: shadingNormal against RT64_IMAGE_SHADING_NORMAL (SNORM16, then RGBA16F) and position against
    RT64_IMAGE_SHADING_POSITION (origin + t direction of the frame's own ray)."""
    from sm64rt_legacy_renderer_amd import rt64
    data = copy.copy(sample_data)
    data.shader_flags = sample_data.shader_flags & ~rt64.SHADER_NORMAL_MAP_ENABLED
    assert all(i.material.depthBias == 0.0 for i in data.instances)
    s = _open(rt64_lib, data, {"lean_frames": 0})
    try:
        s.draw()
        hit = s.readback(rt64.IMAGE_PRIMARY_HIT)
        normal = s.readback(rt64.IMAGE_SHADING_NORMAL)[..., :3].astype(np.float64)
        position = s.readback(rt64.IMAGE_SHADING_POSITION)[..., :3].astype(np.float64)
        inst = np.where(hit[..., 3] == 0xFFFFFFFF, -1, (hit[..., 3] >> 24).astype(np.int64))
        pad = np.pad(inst, 3, mode="edge")
        interior = inst >= 0
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                interior &= pad[3 + dy:3 + dy + H, 3 + dx:3 + dx + W] == inst
        ys, xs = np.nonzero(interior)
        assert len(xs) >= 40 and len(set(inst[ys, xs].tolist())) == 2          # the sphere and the floor
        rays = ray_rule.camera_rays(data, W, H, np.stack([xs, ys], axis=1))
        hits, got = rt64.trace_surfaces(rt64_lib, s.view, rays)
    finally:
        s.close()
    rule, real = _held_to_the_rule("camera rays", data, rays, hits, got, say=False)
    assert real.all() and np.array_equal(hits.view(np.int32)[:, 3], inst[ys, xs])
    dn = np.abs(got[:, 8:11].astype(np.float64) - normal[ys, xs])
    print("shading normal against the image: max %.3e (allowed %.3e + the rule's bound, at most %.1e)" % (dn.max(), 2.0 ** -11 + 2.0 ** -16, rule["shading"][1].max()))
    assert (dn <= 2.0 ** -11 + 2.0 ** -16 + rule["shading"][1]).all()
    scale = np.maximum(np.abs(position[ys, xs]).max(axis=1), np.abs(rays[:, 0:3]).max(axis=1).astype(np.float64))
    dp = np.abs(got[:, 0:3].astype(np.float64) - position[ys, xs]).max(axis=1) / scale
    print("position against the image: max %.3e of the largest coordinate" % dp.max())
    assert dp.max() < 1e-4


def test_the_forms_agree_byte_for_byte(rt64_lib, sample_data):
    """3.  RT64_TraceViewRaySurfaces = RT64_TraceViewRays then RT64_ResolveViewRayHits; the device form on the device's stream and on a caller stream gives the
    same records; also for an accept-first, back-face-culling query."""
    from sm64rt_legacy_renderer_amd import rt64
    s = _open(rt64_lib, sample_data)
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = ray_rule.random_rays(sample_data, 23, 2000, floor_instance=3)
        for flags in (0, rt64.RAY_FLAG_ACCEPT_FIRST_HIT | rt64.RAY_FLAG_CULL_BACK_FACING):
            hits = rt64.trace_rays(rt64_lib, s.view, rays, flags)
            rec = rt64.resolve_hits(rt64_lib, s.view, rays, hits)
            hits2, rec2 = rt64.trace_surfaces(rt64_lib, s.view, rays, flags)
            assert np.array_equal(_bits(hits), _bits(hits2)) and np.array_equal(_bits(rec), _bits(rec2))
            rec3 = np.full_like(rec, 7.0)          # hits = NULL is allowed
            assert rt64_lib.TraceViewRaySurfaces(s.view, rays.ctypes.data, None, rec3.ctypes.data, len(rays), flags) == 1, rt64_lib.last_error()
            assert np.array_equal(_bits(rec), _bits(rec3))
            d_rays, d_hits, d_rec = hip.upload(rays), hip.upload(hits), hip.alloc(rec.nbytes)
            assert rt64_lib.ResolveViewRayHitsDevice(s.view, d_rays, d_hits, d_rec, len(rays), None) == 1, rt64_lib.last_error()
            assert np.array_equal(_bits(hip.download(d_rec, rec)), _bits(rec))
            d_rec2, st = hip.alloc(rec.nbytes), hip.stream()
            assert rt64_lib.ResolveViewRayHitsDevice(s.view, d_rays, d_hits, d_rec2, len(rays), st) == 1, rt64_lib.last_error()
            assert hip.h.hipStreamSynchronize(st) == 0
            assert np.array_equal(_bits(hip.download(d_rec2, rec)), _bits(rec))
            assert (hits.view(np.int32)[:, 3] >= 0).sum() > 100
    finally:
        hip.close()
        s.close()


def test_grid_stride_and_the_end_of_the_array(rt64_lib, sample_data):
    """4.  600 000 records in one launch (more than the 2048 x 256 lanes of its grid): every repetition of the 2000-ray batch equals the first, on the device form
    and through the host form's chunks.  Counts 1, 63, 64, 65, 257 leave the bytes behind the last record as they were."""
    from sm64rt_legacy_renderer_amd import rt64
    s = _open(rt64_lib, sample_data)
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = ray_rule.random_rays(sample_data, 29, 2000, floor_instance=3)
        hits = rt64.trace_rays(rt64_lib, s.view, rays)
        first = rt64.resolve_hits(rt64_lib, s.view, rays, hits)
        reps = 300
        many_rays, many_hits = np.ascontiguousarray(np.tile(rays, (reps, 1))), np.ascontiguousarray(np.tile(hits, (reps, 1)))
        n = len(many_rays)
        assert n == 600000 and n > 2048 * 256
        like = np.empty((n, 16), dtype=np.float32)
        d_rays, d_hits, d_rec = hip.upload(many_rays), hip.upload(many_hits), hip.alloc(like.nbytes)
        assert rt64_lib.ResolveViewRayHitsDevice(s.view, d_rays, d_hits, d_rec, n, None) == 1, rt64_lib.last_error()
        got = _bits(hip.download(d_rec, like)).reshape(reps, len(rays), 16)
        assert (got == _bits(first)[None]).all()
        host = _bits(rt64.resolve_hits(rt64_lib, s.view, many_rays, many_hits)).reshape(reps, len(rays), 16)
        assert (host == _bits(first)[None]).all()
        # sorted by instance, every wave's hits lie on one instance (the kernel's scalar path); in the order given they are mixed (per-lane gathers): same records
        order = np.argsort(hits.view(np.int32)[:, 3], kind="stable")
        assert np.array_equal(_bits(rt64.resolve_hits(rt64_lib, s.view, rays[order], hits[order])), _bits(first)[order])
        guard = np.full((258, 16), 0xABABABAB, dtype=np.uint32)
        for count in (1, 63, 64, 65, 257):
            d_guard = hip.upload(guard)
            assert rt64_lib.ResolveViewRayHitsDevice(s.view, d_rays, d_hits, d_guard, count, None) == 1
            out = hip.download(d_guard, guard)
            assert np.array_equal(out[:count], _bits(first)[:count]) and (out[count:] == 0xABABABAB).all(), count
            h_guard = guard.copy()
            assert rt64_lib.ResolveViewRayHits(s.view, rays.ctypes.data, hits.ctypes.data, h_guard.ctypes.data, count) == 1
            assert np.array_equal(h_guard[:count], _bits(first)[:count]) and (h_guard[count:] == 0xABABABAB).all(), count
    finally:
        hip.close()
        s.close()


def _moved(inst, dx):
    i = copy.copy(inst)
    t = np.array(inst.transform, dtype=np.float32).copy(); t[3, 0] += np.float32(dx)
    i.transform = t; i.previous_transform = t
    return i


def test_misses_bad_hits_and_refusals(rt64_lib, sample_data):
    """5.  A2: misses give the miss record.  A3: instance = instanceCount and primitive = triCount give BAD_HIT records and the call succeeds.  A9: every refusal
    returns 0 with a message that names the function; count = 0 succeeds and touches nothing."""
    from sm64rt_legacy_renderer_amd import rt64
    data = copy.copy(sample_data); data.instances = list(sample_data.instances)
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    try:
        rays = ray_rule.random_rays(data, 31, 600, floor_instance=3)
        hits = np.zeros_like(rays); hits.view(np.int32)[:, 3] = -1
        rec = np.full((len(rays), 16), 0xABABABAB, dtype=np.uint32)
        R = rt64_lib

        def refused(word, fn="RT64_ResolveViewRayHits", call=None):
            ok = call() if call else R.ResolveViewRayHits(s.view, rays.ctypes.data, hits.ctypes.data, rec.ctypes.data, len(rays))
            assert ok == 0 and fn + ":" in R.last_error() and word in R.last_error(), (ok, R.last_error())
        refused("draw")                                                                   # before the first frame
        refused("draw", "RT64_TraceViewRaySurfaces", lambda: R.TraceViewRaySurfaces(s.view, rays.ctypes.data, hits.ctypes.data, rec.ctypes.data, len(rays), 0))
        assert (rec == 0xABABABAB).all()
        s.draw()
        hits = rt64.trace_rays(R, s.view, rays)
        hi = hits.view(np.int32)
        real, miss = np.nonzero(hi[:, 3] >= 0)[0], np.nonzero(hi[:, 3] < 0)[0]
        assert len(real) > 30 and len(miss) > 30
        edited = hits.copy(); ei = edited.view(np.int32)
        rt = S.raytraced_instances(data)
        ei[real[0], 3] = len(rt)                                                          # just past the end, nothing wilder
        tri_count = len(data.meshes[data.instances[rt[int(hi[real[1], 3])]].mesh].indices) // 3
        ei[real[1], 4] = tri_count
        got = rt64.resolve_hits(R, s.view, rays, edited)
        rule, is_real = _held_to_the_rule("edited hits", data, rays, edited, got, say=False)
        gi = _bits(got)
        assert not is_real[real[0]] and not is_real[real[1]] and is_real[real[2:]].all()
        for rows, flags in ((miss, 0), (real[:2], S.BAD_HIT)):
            assert (gi[rows, 3] == flags).all() and (gi[rows, 7] == 0xFFFFFFFF).all() and (gi[rows, 11] == 0xFFFFFFFF).all()
            assert np.isposinf(got[rows, 14]).all() and not gi[rows][:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 15]].any()
        assert (gi[real[2:], 3] & S.VALID).all()
        # count = 0 succeeds and touches nothing; NULL arrays, a NULL view, unknown flags and misaligned device arrays are refused
        rec[:] = 0xABABABAB
        assert R.ResolveViewRayHits(s.view, rays.ctypes.data, hits.ctypes.data, rec.ctypes.data, 0) == 1
        assert R.TraceViewRaySurfaces(s.view, rays.ctypes.data, None, rec.ctypes.data, 0, 0) == 1
        assert (rec == 0xABABABAB).all()
        refused("NULL", call=lambda: R.ResolveViewRayHits(s.view, None, hits.ctypes.data, rec.ctypes.data, 4))
        refused("NULL", call=lambda: R.ResolveViewRayHits(s.view, rays.ctypes.data, None, rec.ctypes.data, 4))
        refused("NULL", call=lambda: R.ResolveViewRayHits(s.view, rays.ctypes.data, hits.ctypes.data, None, 4))
        refused("NULL view", call=lambda: R.ResolveViewRayHits(None, rays.ctypes.data, hits.ctypes.data, rec.ctypes.data, 4))
        refused("NULL", "RT64_TraceViewRaySurfaces", lambda: R.TraceViewRaySurfaces(s.view, rays.ctypes.data, hits.ctypes.data, None, 4, 0))
        refused("unknown flags", "RT64_TraceViewRaySurfaces", lambda: R.TraceViewRaySurfaces(s.view, rays.ctypes.data, hits.ctypes.data, rec.ctypes.data, 4, 0x100))
        d_rays, d_hits, d_rec = hip.upload(rays), hip.upload(hits), hip.alloc(rec.nbytes)
        dev = "RT64_ResolveViewRayHitsDevice"
        refused("NULL", dev, lambda: R.ResolveViewRayHitsDevice(s.view, d_rays, None, d_rec, 4, None))
        refused("NULL", dev, lambda: R.ResolveViewRayHitsDevice(s.view, d_rays, d_hits, None, 4, None))
        for a, b, c in ((d_rays + 4, d_hits, d_rec), (d_rays, d_hits + 8, d_rec), (d_rays, d_hits, d_rec + 4)):
            refused("aligned", dev, lambda: R.ResolveViewRayHitsDevice(s.view, a, b, c, 4, None))
        assert (rec == 0xABABABAB).all()
        # RT64_SetMesh on a mesh the frame traced (same arrays), then RT64_DestroyMesh on one (its instance goes first): refused until the next frame
        m = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], m.vertices, m.indices)
        refused("RT64_SetMesh")
        refused("RT64_SetMesh", dev, lambda: R.ResolveViewRayHitsDevice(s.view, d_rays, d_hits, d_rec, 4, None))
        s.draw()
        assert np.array_equal(_bits(rt64.resolve_hits(R, s.view, rays, edited)), gi)
        mh = R.CreateMesh(s.device, m.flags)
        s.set_mesh(mh, m.vertices, m.indices); s.meshes.append(mh)
        ih = R.CreateInstance(s.scene); s.instances.append(ih)
        from sm64rt_legacy_renderer_amd import sample_scene
        far = _moved(data.instances[1], -3.0)
        s.set_instance(len(s.instances) - 1, sample_scene.InstanceData("extra", len(s.meshes) - 1, far.transform, far.transform, far.diffuse, None, None, far.material))
        s.draw()
        R.DestroyInstance(ih); s.instances.pop()
        R.DestroyMesh(mh); s.meshes.pop()
        refused("destroyed")
        s.draw()
        assert np.array_equal(_bits(rt64.resolve_hits(R, s.view, rays, edited)), gi)
    finally:
        hip.close()
        s.close()


def test_resolve_on_a_caller_stream_describes_the_frame_it_follows(rt64_lib, sample_data):
    """5, last item.  Enqueued on a caller's stream right after a frame, then the sphere moves and the next frame is drawn at once: the records are those of the
    first frame (its table slot, vertex and index arrays are held until the resolve has run); a resolve after the second frame describes the second."""
    from sm64rt_legacy_renderer_amd import rt64
    data = copy.copy(sample_data); data.instances = list(sample_data.instances)
    s = _open(rt64_lib, data, {"sync_present": 0})
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = ray_rule.random_rays(data, 21, 2000, floor_instance=3)
        hits = rt64.trace_rays(rt64_lib, s.view, rays)
        first = rt64.resolve_hits(rt64_lib, s.view, rays, hits)
        _held_to_the_rule("first frame", data, rays, hits, first, say=False)
        reps = 64
        many_rays, many_hits = np.ascontiguousarray(np.tile(rays, (reps, 1))), np.ascontiguousarray(np.tile(hits, (reps, 1)))
        like = np.empty((len(many_rays), 16), dtype=np.float32)
        d_rays, d_hits, d_rec = hip.upload(many_rays), hip.upload(many_hits), hip.alloc(like.nbytes)
        st = hip.stream()
        assert rt64_lib.ResolveViewRayHitsDevice(s.view, d_rays, d_hits, d_rec, len(many_rays), st) == 1, rt64_lib.last_error()
        data.instances[1] = _moved(data.instances[1], 1.5)       # Rt64Scene.draw hands the sphere's description to the library
        s.draw()
        got = _bits(hip.download(d_rec, like)).reshape(reps, len(rays), 16)
        assert (got == _bits(first)[None]).all()
        # the same hit records after the second frame: the sphere's points have moved with it
        second = rt64.resolve_hits(rt64_lib, s.view, rays, hits)
        _held_to_the_rule("second frame", data, rays, hits, second, say=False)
        sph = hits.view(np.int32)[:, 3] == 0
        assert sph.sum() > 50 and np.allclose(second[sph, 0] - first[sph, 0], 1.5, atol=1e-5) and np.array_equal(_bits(second)[~sph], _bits(first)[~sph])
    finally:
        hip.close()
        s.close()


def test_resolves_between_frames_leave_the_frames_alone(rt64_lib, sample_data):
    """6.  A GI + denoiser sequence with resolves between its frames -- host arrays, and device arrays on a caller stream -- renders byte-identical images to the
    same sequence without them, and a plain query answers the same."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    rays = ray_rule.random_rays(sample_data, 51, 2000, floor_instance=3)
    images = (rt64.IMAGE_FINAL_RGBA8, rt64.IMAGE_OUTPUT_RGBA32F, rt64.IMAGE_INDIRECT_LIGHT_FILTERED, rt64.IMAGE_PRIMARY_HIT)

    def run(resolve):
        data = copy.copy(sample_data)
        s = sample_scene.Rt64Scene(rt64_lib, data, 96, 64, hip_device=0)
        hip = ray_rule.Hip()
        try:
            s.set_view_description(gi_samples=1, denoiser=True)
            assert s.option("denoiser_mode", 1)
            out = []
            st = hip.stream()
            d_rays, d_hits, d_rec = hip.upload(rays), hip.alloc(rays.nbytes), hip.alloc(len(rays) * REC)
            for f in range(3):
                v = np.array(sample_data.view, dtype=np.float32).copy(); v[3, 0] += np.float32(0.05 * f)
                data.view = v
                s.draw()
                hits = rt64.trace_rays(rt64_lib, s.view, rays)
                if resolve:
                    rt64.resolve_hits(rt64_lib, s.view, rays, hits)
                    rt64.trace_surfaces(rt64_lib, s.view, rays, rt64.RAY_FLAG_CULL_BACK_FACING)
                    assert hip.h.hipMemcpy(d_hits, hits.ctypes.data, hits.nbytes, 1) == 0
                    assert rt64_lib.ResolveViewRayHitsDevice(s.view, d_rays, d_hits, d_rec, len(rays), st) == 1
                out.append([s.readback(k).copy() for k in images] + [hits])
            return out
        finally:
            hip.close()
            s.close()
    a, b = run(False), run(True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert x.tobytes() == y.tobytes()
