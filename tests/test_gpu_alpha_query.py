"""Ray queries that honour alpha (RT64_TraceViewRaysAlpha, RT64_TraceViewRayVisibility, include/rt64_alpha.h) on the GPU, held to the float64 rule of
tests/alpha_rule.py ray by ray (rules K1-K10), to the walk that commits everything (K8), to the frame's own instance image, to the two-step workaround
they replace, and to themselves: the forms agree byte for byte, the grid-stride loop repeats itself exactly, nothing is written past the last record, bad calls are
refused as K9 says, a destroyed texture waits for an enqueued query, and frames do not notice.

The candidates of every ray come from the oracle's enumeration (tests/alpha_rule.py), their alphas from tests/material_rule.py.  One run's lines of the first test
are committed as profiles/alpha_rule_deviation.txt.
"""
import copy

import numpy as np
import pytest

import alpha_cases as AC
import alpha_rule as R
import material_cases as MC
import material_rule as M
import ray_rule
from test_alpha_rule import MUTATION_CASES

pytestmark = pytest.mark.gpu

W, H = 64, 36
CULL, FIRST = R.CULL_BACK_FACING, R.ACCEPT_FIRST_HIT


def _open(rt64_lib, data, options=None, w=W, h=H):
    from sm64rt_legacy_renderer_amd import sample_scene
    options = dict(options or {})
    first = {k: options.pop(k) for k in ("generate_mipmaps",) if k in options}          # applies to textures created while it is set
    s = sample_scene.Rt64Scene(rt64_lib, data, w, h, hip_device=0, options=first)
    for k, v in options.items():
        assert s.option(k, v), k
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _enumerate(data, rays, culls=(0, 1)):
    from oracle import oracle_py
    o = oracle_py.OracleScene(data)
    try:
        o.render(W, H, images=False)
        return {c: R.candidates(o, rays, cull=bool(c)) for c in culls}
    finally:
        o.close()


@pytest.fixture(scope="module")
def cases(sample_data):
    return {name: (data, seed, options, heights) for name, data, seed, options, heights in AC.cases(sample_data)}


@pytest.mark.parametrize("name", AC.NAMES)
def test_the_walks_lie_within_the_rule_ray_by_ray(rt64_lib, oracle_lib, cases, name):
    """1.  K2 with the case's lods: t, u, v bit-equal and instance, primitive exact on every decided ray, with and without back-face culling; under ACCEPT_FIRST_HIT a
    member of the accepted set, a miss exactly where that is empty.  K5: |visibility - rule| <= bound on every decided ray, flags exact where the rule's interval
    excludes 0 or is 0 exactly, undecided rays finite and in 0 .. 1.  The mutations assigned to the case leave their own bound against these results."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, heights = cases[name]
    rays = AC.rays_of(data, seed, heights)
    lods = AC.lods_of(seed, len(rays), options)
    s = _open(rt64_lib, data, options)
    try:
        s.draw()
        got = {f: rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods, f) for f in (0, CULL, FIRST, CULL | FIRST)}
        vis = rt64.trace_visibility(rt64_lib, s.view, rays)
        vis_cull = rt64.trace_visibility(rt64_lib, s.view, rays, CULL)
    finally:
        s.close()
    levels = M.texture_levels(data, MC.mipmapped(options))
    cand = _enumerate(data, rays)
    rules = {flags: R.closest_hit(data, levels, rays, cand[c], lods) for c, flags in ((0, 0), (1, CULL))}
    k2 = {}          # flags -> rays that miss K2: measured first, printed, then held
    for flags, rule in rules.items():
        k2[flags] = ~R.closest_matches(rule, got[flags])
        k2[flags | FIRST] = ~R.first_matches(rule, got[flags | FIRST])
    closest = rules[0]
    v = R.visibility(data, levels, rays, cand[0])
    ratio, ok = R.visibility_check(v, vis)
    decided = ~v["undecided"]
    print("%-40s rays %4d  K2 hits %4d closest candidate cut out %4d undecided %.4f mismatches %d (of 4 x %d)  K5 below 1: %4d largest ratio %.3f largest bound %.2e undecided %.4f" %
          (name, len(rays), int((_bits(got[0])[:, 3] != 0xFFFFFFFF).sum()), int(closest["cutout_first"].sum()), closest["undecided"].mean(),
           sum(int(m.sum()) for m in k2.values()), len(rays), int((vis[:, 0] < 1.0).sum()), ratio.max(), v["e"].max(), v["undecided"].mean()))
    for flags, rule in rules.items():
        assert rule["undecided"].mean() <= 0.02
    for flags, miss in k2.items():
        assert not miss.any(), (name, flags, np.nonzero(miss)[0][:8].tolist())
    assert v["undecided"].mean() <= 0.02 and v["e"].max() <= 1e-4
    assert ok.all(), (name, np.nonzero(~ok)[0][:8].tolist())
    assert (ratio[decided] <= 1.0).all(), (name, float(ratio.max()), np.nonzero(~(ratio <= 1.0))[0][:8].tolist())
    ratio_c, ok_c = R.visibility_check(R.visibility(data, levels, rays, cand[1]), vis_cull)          # K3: the one flag a visibility query takes
    assert ok_c.all() and (ratio_c <= 1.0).all(), name
    for mutation, where in MUTATION_CASES.items():
        if where != name:
            continue
        if mutation in R.CLOSEST_MUTATIONS:
            out = ~R.closest_matches(R.closest_hit(data, levels, rays, cand[0], lods, mutate=mutation), got[0])
        else:
            m = R.visibility(data, levels, rays, cand[1 if mutation == "shadows_cull_back_faces" else 0], mutate=mutation, lods=lods)
            mr, mok = R.visibility_check(m, vis)
            out = ~mok | ~(mr <= 1.0)
        print("    mutation %-28s %4d of %4d of the device's rays outside its bound" % (mutation, int(out.sum()), len(out)))
        assert out.sum() >= 1, mutation


def test_the_equivalences_hold_on_the_device(rt64_lib, sample_data):
    """2.  K8, byte for byte: without a texture-edge shader the alpha walk returns RT64_TraceViewRays' t, u, v, instance, primitive under every flag combination (the
    sample scene, the combiner cases without an edge shader, lods or not); on the sample scene, all O2-opaque, visibility is 0 exactly where the accept-first walk
    hits and 1 where it misses."""
    from sm64rt_legacy_renderer_amd import rt64
    scenes = [("sample", MC.small_sample(sample_data), {"lds_cache": 1}), ("sample from HBM", MC.small_sample(sample_data), {"lds_cache": 0})]
    scenes += [(n, MC.combiner_case(sample_data, n, sid, smp), {}) for n, sid, smp in MC.COMBINERS if not sid & MC.OPT_EDGE]
    assert len(scenes) == 9
    for k, (name, data, options) in enumerate(scenes):
        rays = ray_rule.random_rays(data, 300 + k, 2000, floor_instance=3)
        lods = MC.lods(300 + k, len(rays), False)
        s = _open(rt64_lib, data, options)
        try:
            s.draw()
            for flags in (0, CULL, FIRST, CULL | FIRST):
                plain = rt64.trace_rays(rt64_lib, s.view, rays, flags)
                for l in (None, lods):
                    assert np.array_equal(_bits(rt64.trace_rays_alpha(rt64_lib, s.view, rays, l, flags))[:, :5], _bits(plain)[:, :5]), (name, flags)
                assert (_bits(plain)[:, 3] != 0xFFFFFFFF).sum() > 100
            if k < 2:
                hit = _bits(rt64.trace_rays(rt64_lib, s.view, rays, FIRST))[:, 3] != 0xFFFFFFFF
                vis = rt64.trace_visibility(rt64_lib, s.view, rays)
                valid = np.array([ray_rule.ray_is_valid(r) for r in rays])
                assert np.array_equal(vis[:, 0], np.where(hit, 0.0, 1.0).astype(np.float32)), name
                assert np.array_equal(_bits(vis)[:, 1], np.where(hit, 3, np.where(valid, 1, 0))), name
                assert hit.sum() > 100 and (~hit).sum() > 100
        finally:
            s.close()


def test_camera_rays_agree_with_the_frame(rt64_lib, oracle_lib, sample_data):
    """3.  The fence, every G-buffer image written (lean_frames = 0): the instance K2 names for the camera ray of a pixel is RT64_IMAGE_PRIMARY_HIT's on every decided
    pixel."""
    from sm64rt_legacy_renderer_amd import rt64
    data = AC.fence(sample_data)
    px = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="xy"), axis=-1).reshape(-1, 2)
    rays = ray_rule.camera_rays(data, W, H, px)
    s = _open(rt64_lib, data, {"lean_frames": 0})
    try:
        s.draw()
        hit = s.readback(rt64.IMAGE_PRIMARY_HIT)
        got = rt64.trace_rays_alpha(rt64_lib, s.view, rays, None, CULL)
        plain = rt64.trace_rays(rt64_lib, s.view, rays, CULL)
    finally:
        s.close()
    shown = np.where(hit[..., 3] == 0xFFFFFFFF, -1, (hit[..., 3] >> 24).astype(np.int64)).reshape(-1)
    rule = R.closest_hit(data, M.texture_levels(data), rays, _enumerate(data, rays, (1,))[1])
    decided = ~rule["undecided"]
    mine = got.view(np.int32)[:, 3]
    assert decided.mean() >= 0.98 and len(set(mine[decided].tolist())) >= 4
    assert np.array_equal(mine[decided], shown[decided]), np.nonzero(decided & (mine != shown))[0][:8].tolist()
    assert (plain.view(np.int32)[:, 3] != shown).sum() >= 100          # the walk that commits everything names the hole's layer instead


@pytest.mark.parametrize("name", AC.FENCES)
def test_one_call_equals_the_two_step_workaround(rt64_lib, cases, name):
    """4.  Trace, shade, trace again the rays whose hit is flagged RT64_MATERIAL_CUTOUT from tMin = t, until none is flagged: the hits of one RT64_TraceViewRaysAlpha
    call, t, u, v, instance, primitive byte for byte."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, heights = cases[name]
    rays = AC.rays_of(data, seed, heights)
    lods = AC.lods_of(seed, len(rays), options)
    s = _open(rt64_lib, data, options)
    try:
        s.draw()
        for flags in (0, CULL):
            got = rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods, flags)
            cur = rays.copy(); hits = rt64.trace_rays(rt64_lib, s.view, cur, flags); rounds = 0
            while True:
                cut = (_bits(rt64.shade_hits(rt64_lib, s.view, cur, hits, lods))[:, 7] & M.CUTOUT) != 0
                if not cut.any():
                    break
                rounds += 1
                cur[cut, 3] = hits[cut, 0]
                hits[cut] = rt64.trace_rays(rt64_lib, s.view, cur[cut], flags)
            assert rounds >= 2 and np.array_equal(_bits(got)[:, :5], _bits(hits)[:, :5]), (name, flags, rounds)
    finally:
        s.close()


def test_the_forms_agree_byte_for_byte(rt64_lib, sample_data):
    """5.  Host arrays, device arrays on the device's stream and on a caller stream: the same records; lods = NULL is an array of zeros."""
    from sm64rt_legacy_renderer_amd import rt64
    data = AC.fence(sample_data)
    s = _open(rt64_lib, data, {"generate_mipmaps": 1})
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = AC.rays_of(data, 23, AC.FENCE_HEIGHTS)
        lods = MC.lods(23, len(rays), True)
        d_rays, d_lods = hip.upload(rays), hip.upload(lods)
        for flags, l, d_l in ((0, None, None), (0, lods, d_lods), (FIRST | CULL, lods, d_lods)):
            host = rt64.trace_rays_alpha(rt64_lib, s.view, rays, l, flags)
            assert (_bits(host)[:, 3] != 0xFFFFFFFF).sum() > 100
            for st in (None, hip.stream()):
                d_hits = hip.alloc(host.nbytes)
                assert rt64_lib.TraceViewRaysAlphaDevice(s.view, d_rays, d_l, d_hits, len(rays), flags, st) == 1, rt64_lib.last_error()
                if st:
                    assert hip.h.hipStreamSynchronize(st) == 0
                assert np.array_equal(_bits(hip.download(d_hits, host)), _bits(host))
            if l is None:
                assert np.array_equal(_bits(rt64.trace_rays_alpha(rt64_lib, s.view, rays, np.zeros(len(rays), dtype=np.float32), flags)), _bits(host))
        for flags in (0, CULL):
            host = rt64.trace_visibility(rt64_lib, s.view, rays, flags)
            assert ((host[:, 0] > 0.0) & (host[:, 0] < 1.0)).sum() > 100
            for st in (None, hip.stream()):
                d_vis = hip.alloc(host.nbytes)
                assert rt64_lib.TraceViewRayVisibilityDevice(s.view, d_rays, d_vis, len(rays), flags, st) == 1, rt64_lib.last_error()
                if st:
                    assert hip.h.hipStreamSynchronize(st) == 0
                assert np.array_equal(_bits(hip.download(d_vis, host)), _bits(host))
    finally:
        hip.close()
        s.close()


def test_sizes_grid_stride_and_the_end_of_the_array(rt64_lib, sample_data):
    """6.  Counts 1, 63, 64, 65, 255, 256, 257 and RT_GRID_BLOCKS x RT_BLOCK + 65 (the grid-stride loop): each equals the prefix of one big call, on the device forms
    (guard words behind the last record untouched: 32-byte hits and 16-byte visibility records) and on the host forms."""
    from sm64rt_legacy_renderer_amd import rt64
    data = AC.fence(sample_data)
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays = AC.rays_of(data, 29, AC.FENCE_HEIGHTS)
        big = 2048 * 256 + 65
        reps = -(-(big + 300) // len(rays))
        rng = np.random.default_rng(5)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(reps - 1)])          # later repetitions shuffled: waves mix instances
        many = np.ascontiguousarray(rays[order])
        n = len(many)
        assert big > 2048 * 256 and n >= big + 258
        whole = {8: _bits(rt64.trace_rays_alpha(rt64_lib, s.view, many)), 4: _bits(rt64.trace_visibility(rt64_lib, s.view, many))}          # host forms: chunks of 2^20
        first = {8: _bits(rt64.trace_rays_alpha(rt64_lib, s.view, rays)), 4: _bits(rt64.trace_visibility(rt64_lib, s.view, rays))}
        for words in (8, 4):
            assert np.array_equal(whole[words], first[words][order]), words          # a ray's record does not depend on its place or its neighbours
        d_rays = hip.upload(many)
        for words in (8, 4):
            guard = np.full((n, words), 0xABABABAB, dtype=np.uint32)
            for count in (1, 63, 64, 65, 255, 256, 257, big):
                d_guard = hip.upload(guard[:count + 258])
                if words == 8:
                    assert rt64_lib.TraceViewRaysAlphaDevice(s.view, d_rays, None, d_guard, count, 0, None) == 1, rt64_lib.last_error()
                else:
                    assert rt64_lib.TraceViewRayVisibilityDevice(s.view, d_rays, d_guard, count, 0, None) == 1, rt64_lib.last_error()
                out = hip.download(d_guard, guard[:count + 258])
                assert np.array_equal(out[:count], whole[words][:count]) and (out[count:] == 0xABABABAB).all(), (words, count)
                if count <= 257:
                    h_guard = guard[:count + 258].copy()
                    if words == 8:
                        assert rt64_lib.TraceViewRaysAlpha(s.view, many.ctypes.data, None, h_guard.ctypes.data, count, 0) == 1
                    else:
                        assert rt64_lib.TraceViewRayVisibility(s.view, many.ctypes.data, h_guard.ctypes.data, count, 0) == 1
                    assert np.array_equal(h_guard[:count], whole[words][:count]) and (h_guard[count:] == 0xABABABAB).all(), (words, count)
    finally:
        hip.close()
        s.close()


def test_counters_follow_count_traversal(rt64_lib, sample_data):
    """7.  K1: nodesVisited and trianglesTested are 0 without count_traversal; with it, non-zero for the rays that were walked into the scene, the committing walk's
    own on a scene where the any-hit never runs, and 0 for Q6-invalid rays."""
    from sm64rt_legacy_renderer_amd import rt64
    data = MC.small_sample(sample_data)
    rays = ray_rule.random_rays(data, 33, 2000, floor_instance=3)
    rays[5, 4:7] = 0.0; rays[6, 0] = np.nan; rays[7, 3] = 2.0; rays[7, 7] = 1.0          # Q6
    s = _open(rt64_lib, data)
    try:
        s.draw()
        a, v = _bits(rt64.trace_rays_alpha(rt64_lib, s.view, rays)), _bits(rt64.trace_visibility(rt64_lib, s.view, rays))
        assert not a[:, 5:8].any() and not v[:, 2:4].any()
        assert s.option("count_traversal", 1)
        s.draw()
        a, v = _bits(rt64.trace_rays_alpha(rt64_lib, s.view, rays)), _bits(rt64.trace_visibility(rt64_lib, s.view, rays))
        plain, first = _bits(rt64.trace_rays(rt64_lib, s.view, rays)), _bits(rt64.trace_rays(rt64_lib, s.view, rays, FIRST))
        assert np.array_equal(a, plain) and np.array_equal(v[:, 2:4], first[:, 5:7])
        hit = a[:, 3] != 0xFFFFFFFF
        assert hit.sum() > 100 and (a[hit, 5] > 0).all() and (a[hit, 6] > 0).all() and (v[hit, 2] > 0).all() and (v[hit, 3] > 0).all()
        for k in (5, 6, 7):
            assert not a[k, 5:8].any() and not v[k, 1:4].any() and a[k, 3] == 0xFFFFFFFF and rays[k].size and _bits(np.float32(1.0)) == v[k, 0]
    finally:
        s.close()


def _moved(inst, dx):
    i = copy.copy(inst)
    t = np.array(inst.transform, dtype=np.float32).copy(); t[3, 0] += np.float32(dx)
    i.transform = t; i.previous_transform = t
    return i


def test_refusals(rt64_lib, sample_data):
    """8.  K9, one by one: every refusal returns 0 with a message that names the function; count = 0 succeeds and touches nothing."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    data = MC.small_sample(sample_data)
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    R_ = rt64_lib
    try:
        rays = ray_rule.random_rays(data, 31, 600, floor_instance=3)
        hits = np.full((len(rays), 8), 0xABABABAB, dtype=np.uint32); vis = np.full((len(rays), 4), 0xABABABAB, dtype=np.uint32)
        A, V, AD, VD = "RT64_TraceViewRaysAlpha", "RT64_TraceViewRayVisibility", "RT64_TraceViewRaysAlphaDevice", "RT64_TraceViewRayVisibilityDevice"
        d_rays, d_hits, d_vis, d_lods = hip.upload(rays), hip.alloc(hits.nbytes), hip.alloc(vis.nbytes), hip.upload(np.zeros(len(rays), dtype=np.float32))

        def refused(word, fn, call):
            ok = call()
            assert ok == 0 and fn + ":" in R_.last_error() and word in R_.last_error(), (ok, R_.last_error())

        def all_refused(word):
            refused(word, A, lambda: R_.TraceViewRaysAlpha(s.view, rays.ctypes.data, None, hits.ctypes.data, len(rays), 0))
            refused(word, V, lambda: R_.TraceViewRayVisibility(s.view, rays.ctypes.data, vis.ctypes.data, len(rays), 0))
            refused(word, AD, lambda: R_.TraceViewRaysAlphaDevice(s.view, d_rays, None, d_hits, 4, 0, None))
            refused(word, VD, lambda: R_.TraceViewRayVisibilityDevice(s.view, d_rays, d_vis, 4, 0, None))
        all_refused("draw")                                                               # before the first frame
        s.draw()
        want_a, want_v = rt64.trace_rays_alpha(R_, s.view, rays), rt64.trace_visibility(R_, s.view, rays)
        # count = 0 succeeds and touches nothing
        assert R_.TraceViewRaysAlpha(s.view, rays.ctypes.data, None, hits.ctypes.data, 0, 0) == 1 and R_.TraceViewRayVisibility(s.view, rays.ctypes.data, vis.ctypes.data, 0, 0) == 1
        # NULL arrays (other than lods), a NULL view, flags, misaligned device arrays
        refused("NULL", A, lambda: R_.TraceViewRaysAlpha(s.view, None, None, hits.ctypes.data, 4, 0))
        refused("NULL", A, lambda: R_.TraceViewRaysAlpha(s.view, rays.ctypes.data, None, None, 4, 0))
        refused("NULL", V, lambda: R_.TraceViewRayVisibility(s.view, None, vis.ctypes.data, 4, 0))
        refused("NULL", V, lambda: R_.TraceViewRayVisibility(s.view, rays.ctypes.data, None, 4, 0))
        refused("NULL view", A, lambda: R_.TraceViewRaysAlpha(None, rays.ctypes.data, None, hits.ctypes.data, 4, 0))
        refused("NULL view", V, lambda: R_.TraceViewRayVisibility(None, rays.ctypes.data, vis.ctypes.data, 4, 0))
        refused("NULL", AD, lambda: R_.TraceViewRaysAlphaDevice(s.view, d_rays, None, None, 4, 0, None))
        refused("NULL", VD, lambda: R_.TraceViewRayVisibilityDevice(s.view, None, d_vis, 4, 0, None))
        refused("unknown flags", A, lambda: R_.TraceViewRaysAlpha(s.view, rays.ctypes.data, None, hits.ctypes.data, 4, 0x4))
        refused("unknown flags", V, lambda: R_.TraceViewRayVisibility(s.view, rays.ctypes.data, vis.ctypes.data, 4, FIRST))          # K3
        refused("unknown flags", VD, lambda: R_.TraceViewRayVisibilityDevice(s.view, d_rays, d_vis, 4, CULL | FIRST, None))
        for a, l, b in ((d_rays + 4, None, d_hits), (d_rays, None, d_hits + 8), (d_rays, d_lods + 2, d_hits)):
            refused("aligned", AD, lambda: R_.TraceViewRaysAlphaDevice(s.view, a, l, b, 4, 0, None))
        for a, b in ((d_rays + 8, d_vis), (d_rays, d_vis + 4)):
            refused("aligned", VD, lambda: R_.TraceViewRayVisibilityDevice(s.view, a, b, 4, 0, None))
        assert R_.TraceViewRaysAlphaDevice(s.view, d_rays, d_lods + 4, d_hits, 4, 0, None) == 1          # lods need 4-byte alignment only
        assert R_.TraceViewRayVisibilityDevice(s.view, d_rays, d_vis + 16, 4, 0, None) == 1              # a visibility record is 16 bytes
        assert (hits == 0xABABABAB).all() and (vis == 0xABABABAB).all()
        # RT64_SetMesh on a mesh the frame traced (same arrays), then RT64_DestroyMesh on one (its instance goes first): refused until the next frame
        m = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], m.vertices, m.indices)
        all_refused("RT64_SetMesh")
        s.draw()
        assert np.array_equal(_bits(rt64.trace_rays_alpha(R_, s.view, rays)), _bits(want_a))
        mh = R_.CreateMesh(s.device, m.flags)
        s.set_mesh(mh, m.vertices, m.indices); s.meshes.append(mh)
        ih = R_.CreateInstance(s.scene); s.instances.append(ih)
        far = _moved(data.instances[1], -3.0)
        s.set_instance(len(s.instances) - 1, sample_scene.InstanceData("extra", len(s.meshes) - 1, far.transform, far.transform, far.diffuse, None, None, far.material))
        s.draw()
        R_.DestroyInstance(ih); s.instances.pop()
        R_.DestroyMesh(mh); s.meshes.pop()
        all_refused("destroyed")
        s.draw()
        assert np.array_equal(_bits(rt64.trace_visibility(R_, s.view, rays)), _bits(want_v))
        # RT64_DestroyTexture of a texture the frame's table holds (a copy of the floor's diffuse map on an extra instance, which goes first)
        t = data.textures[4]
        td = rt64.TEXTURE_DESC(); buf, pitch = t.upload_buffer()
        td.bytes = buf.ctypes.data; td.byteCount = buf.nbytes; td.format = t.format; td.width, td.height, td.rowPitch = t.width, t.height, pitch
        th = R_.CreateTexture(s.device, td)
        assert th, R_.last_error()
        s.textures.append(th)
        ih = R_.CreateInstance(s.scene); s.instances.append(ih)
        s.set_instance(len(s.instances) - 1, sample_scene.InstanceData("extra", data.instances[1].mesh, far.transform, far.transform, len(s.textures) - 1, None, None, far.material))
        s.draw()
        before = rt64.trace_rays(R_, s.view, rays)
        assert rt64.trace_rays_alpha(R_, s.view, rays) is not None and rt64.trace_visibility(R_, s.view, rays) is not None
        R_.DestroyInstance(ih); s.instances.pop()
        R_.DestroyTexture(th); s.textures.pop()
        all_refused("texture")
        assert np.array_equal(_bits(rt64.trace_rays(R_, s.view, rays)), _bits(before))          # the walk that reads no texture still answers
        s.draw()
        assert np.array_equal(_bits(rt64.trace_rays_alpha(R_, s.view, rays)), _bits(want_a)) and np.array_equal(_bits(rt64.trace_visibility(R_, s.view, rays)), _bits(want_v))
    finally:
        hip.close()
        s.close()


def test_visibility_on_a_caller_stream_outlives_its_texture(rt64_lib, sample_data):
    """9.  Enqueued on a caller's stream, followed at once by RT64_DestroyTexture of a texture it reads and by a new frame: the records are the bytes of the
    synchronous call made before it (RT64_DestroyTexture waits for the query), and the frame is the frame of a run without any of this."""
    from sm64rt_legacy_renderer_amd import rt64

    def run(query):
        data = AC.veils(sample_data)
        rays = AC.rays_of(data, 21, AC.VEIL_HEIGHTS)
        s = _open(rt64_lib, data, {"sync_present": 0})
        hip = ray_rule.Hip()
        try:
            t = data.textures[4]
            td = rt64.TEXTURE_DESC(); buf, pitch = t.upload_buffer()
            td.bytes = buf.ctypes.data; td.byteCount = buf.nbytes; td.format = t.format; td.width, td.height, td.rowPitch = t.width, t.height, pitch
            th = rt64_lib.CreateTexture(s.device, td)
            s.textures.append(th)
            top = len(data.instances) - 2                                  # a veil over texture 4 ...
            assert data.instances[top].diffuse == 4
            veil = copy.copy(data.instances[top]); veil.diffuse = len(s.textures) - 1          # ... reads the copy instead
            s.set_instance(top, veil)
            s.draw()
            first = None
            if query:
                first = rt64.trace_visibility(rt64_lib, s.view, rays)
                assert ((first[:, 0] > 0.0) & (first[:, 0] < 1.0)).sum() > 100
                reps = 64
                many = np.ascontiguousarray(np.tile(rays, (reps, 1)))
                like = np.empty((len(many), 4), dtype=np.float32)
                d_rays, d_vis = hip.upload(many), hip.alloc(like.nbytes)
                st = hip.stream()
                assert rt64_lib.TraceViewRayVisibilityDevice(s.view, d_rays, d_vis, len(many), 0, st) == 1, rt64_lib.last_error()
            s.set_instance(top, data.instances[top])                     # the veil goes back to the scene's own texture ...
            rt64_lib.DestroyTexture(th); s.textures.pop()                # ... and the copy goes at once
            s.draw()
            if query:
                got = _bits(hip.download(d_vis, like)).reshape(reps, len(rays), 4)
                assert (got == _bits(first)[None]).all()
            return [s.readback(k).copy() for k in (rt64.IMAGE_FINAL_RGBA8, rt64.IMAGE_OUTPUT_RGBA32F, rt64.IMAGE_PRIMARY_HIT)]
        finally:
            hip.close()
            s.close()
    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("streams", [1, 3])
def test_alpha_queries_between_frames_leave_the_frames_alone(rt64_lib, sample_data, streams, monkeypatch):
    """10.  A GI + denoiser sequence with alpha and visibility queries between its frames -- host arrays, and device arrays on a caller stream -- renders byte-identical
    images to the same sequence without them, on one render stream and on three (RT64_RENDER_STREAMS, read when the device is created; frames enqueued)."""
    monkeypatch.setenv("RT64_RENDER_STREAMS", str(streams))
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    rays = ray_rule.random_rays(sample_data, 51, 2000, floor_instance=3)
    lods = MC.lods(51, len(rays), True)
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
            d_rays, d_hits, d_lods, d_vis = hip.upload(rays), hip.alloc(rays.nbytes), hip.upload(lods), hip.alloc(len(rays) * 16)
            for f in range(3):
                v = np.array(sample_data.view, dtype=np.float32).copy(); v[3, 0] += np.float32(0.05 * f)
                data.view = v
                s.draw()
                hits = rt64.trace_rays(rt64_lib, s.view, rays)
                if query:
                    rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods, CULL)
                    rt64.trace_visibility(rt64_lib, s.view, rays)
                    assert rt64_lib.TraceViewRaysAlphaDevice(s.view, d_rays, d_lods, d_hits, len(rays), 0, st) == 1
                    assert rt64_lib.TraceViewRayVisibilityDevice(s.view, d_rays, d_vis, len(rays), 0, st) == 1
                out.append([s.readback(k).copy() for k in images] + [hits])
            return out
        finally:
            hip.close()
            s.close()
    a, b = run(False), run(True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert x.tobytes() == y.tobytes()
