"""Camera rays and texture footprints of ray-query hits (RT64_GenerateViewCameraRays, RT64_FootprintViewRayHits, RT64_TraceViewPixelFootprints,
include/rt64_footprint.h) on the GPU, held to the float64 rule of tests/footprint_rule.py (rules F1-F11), to the frame's own images, and to
themselves: the forms agree byte for byte, nothing is written past the last record, bad hits and bad calls are answered as F4 / F10 say.

The texture sizes and level counts come from RT64_ReadbackTexture, the walks from the library's own rt64.trace_rays (tests/test_gpu_ray_query.py holds that to
the oracle bit for bit).  One run's lines of the first three tests are committed as profiles/footprint_rule_deviation.txt.
"""
import numpy as np
import pytest

import footprint_cases as FC
import footprint_rule as R
import material_rule as M
import ray_rule

pytestmark = pytest.mark.gpu

HALF_UNORM8, HALF_SNORM16, HALF_F16 = 0.5 / 255.0, 2.0 ** -16, 2.0 ** -11
UNDECIDED_CAP = 0.01          # tests/test_footprint_rule.py holds the rule alone to the same cap


def _open(rt64_lib, case, **more):
    """The case's scene with its frames drawn."""
    from sm64rt_legacy_renderer_amd import sample_scene
    options = dict(case["options"], **more)
    first = {k: options.pop(k) for k in ("generate_mipmaps",) if k in options}          # applies to textures created while it is set
    s = sample_scene.Rt64Scene(rt64_lib, case["data"], case["screen"][0], case["screen"][1], hip_device=0, options=first)
    try:
        for k, v in options.items():
            assert s.option(k, v), k
        if case["view"]:
            s.set_view_description(**case["view"])
        for _ in range(case["frames"]):
            s.draw()
    except Exception:
        s.close()
        raise
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _levels(lib, s, data):
    """texture index -> every level the library holds of it, read back."""
    out = {}
    for k, t in enumerate(data.textures):
        if t.format != 0x1:
            continue
        lv, m = [], 0
        while True:
            n = lib.ReadbackTexture(s.textures[k], m, None, 0)
            if n == 0:
                break
            a = np.zeros((max(1, t.height >> m), max(1, t.width >> m), 4), dtype=np.uint8)
            assert n == a.nbytes and lib.ReadbackTexture(s.textures[k], m, a.ctypes.data, a.nbytes) == a.nbytes, lib.last_error()
            lv.append(a); m += 1
        out[k] = lv
    return out


def _held_to_the_rule(name, data, textures, rays, diffs, hits, got, say=True):
    rule = R.footprints(data, textures, rays, diffs, hits)
    ratios, exact, lods_ok = R.compare(rule, got)
    if say:
        print(R.report(name, rule, ratios, exact, lods_ok))
    assert exact.all(), (name, np.nonzero(~exact)[0][:8].tolist())
    assert lods_ok.all(), (name, np.nonzero(~lods_ok)[0][:8].tolist())
    for k, r in ratios.items():
        assert (r < 1.0).all(), (name, k, float(r.max()), np.nonzero(~(r < 1.0))[0][:8].tolist())
    levels_ok, _ = R.compare_levels(rule, got)          # under a POINT sampler: the level the record's lod selects is the rule's, or either neighbour where undecided
    assert levels_ok.all(), (name, np.nonzero(~levels_ok)[0][:8].tolist())
    return rule


@pytest.fixture(scope="module")
def cases(sample_data):
    return {c["name"]: c for c in FC.cases(sample_data)}


@pytest.mark.parametrize("name", FC.NAMES)
def test_the_rays_are_the_frames(rt64_lib, cases, name):
    """1.  Every pixel of the frame: origin, direction and differential within the rule's bound, tMin / tMax / dO / reserved exact; walked with the frame's culling
    they give t, u, v, instance and primitive of RT64_IMAGE_PRIMARY_HIT bit for bit on every pixel the image calls a hit; pixels = NULL, rays without differentials
    and the device form give the same bytes; coordinates outside the frame follow the rule's extrapolation."""
    from sm64rt_legacy_renderer_amd import rt64
    case = cases[name]
    w, h = case["render"]
    s = _open(rt64_lib, case, lean_frames=0)
    hip = ray_rule.Hip()
    try:
        image = s.readback(rt64.IMAGE_PRIMARY_HIT)
        assert image.shape == (h, w, 4)
        pixels = FC.all_pixels(case)
        rays, diffs = rt64.camera_rays(rt64_lib, s.view, pixels)
        rays2, diffs2 = rt64.camera_rays(rt64_lib, s.view, None, count=w * h)
        only = rt64.camera_rays(rt64_lib, s.view, pixels, differentials=False)
        hits = rt64.trace_rays(rt64_lib, s.view, rays, rt64.RAY_FLAG_CULL_BACK_FACING)
        outside = np.array([[w, 0], [0, h], [w + 9, h + 5], [5000, 3], [7, 4000], [2 * w, 2 * h]], dtype=np.uint32)
        orays, odiffs = rt64.camera_rays(rt64_lib, s.view, outside)
        d_pix, d_rays, d_diffs = hip.upload(pixels), hip.alloc(rays.nbytes), hip.alloc(diffs.nbytes)
        assert rt64_lib.GenerateViewCameraRaysDevice(s.view, d_pix, d_rays, d_diffs, len(pixels), None) == 1, rt64_lib.last_error()
        dev = hip.download(d_rays, rays), hip.download(d_diffs, diffs)
        d_rays2, st = hip.alloc(rays.nbytes), hip.stream()
        assert rt64_lib.GenerateViewCameraRaysDevice(s.view, None, d_rays2, None, len(pixels), st) == 1, rt64_lib.last_error()
        assert hip.h.hipStreamSynchronize(st) == 0
        dev2 = hip.download(d_rays2, rays)
    finally:
        hip.close()
        s.close()
    for a in (rays2, only, dev[0], dev2):
        assert np.array_equal(_bits(a), _bits(rays))
    for a in (diffs2, dev[1]):
        assert np.array_equal(_bits(a), _bits(diffs))
    cam = FC.camera_of(case)
    for tag, px, r, d in (("", pixels, rays, diffs), (" outside", outside, orays, odiffs)):
        ratios, exact = R.compare_rays(R.camera_rays(cam, px), r, d)
        print("%-36s%-8s " % (name, tag) + "  ".join("%s max %.3f" % (k, v.max()) for k, v in ratios.items()))
        assert exact.all(), (name, tag)
        for k, v in ratios.items():
            assert (v < 1.0).all(), (name, tag, k, float(v.max()))
    flat = image.reshape(-1, 4)
    hit = flat[:, 3] != 0xFFFFFFFF
    hu = _bits(hits)
    assert hit.sum() > len(pixels) // 20
    assert np.array_equal(hu[hit, 0:3], flat[hit, 0:3]), name                                        # t, u, v: the same bits
    assert np.array_equal(hu[hit, 3], flat[hit, 3] >> 24) and np.array_equal(hu[hit, 4] & 0xFFFFFF, flat[hit, 3] & 0xFFFFFF), name
    assert (hits.view(np.int32)[~hit, 3] < 0).all(), name                                            # ... and a pixel the frame calls a miss is one


@pytest.mark.parametrize("name", FC.NAMES)
def test_footprints_lie_within_the_rule_hit_by_hit(rt64_lib, cases, name):
    """2.  2000 random rays with random differentials (dO != 0 among them) and the frame's own camera rays: gradients and dPd* within the bound on decided hits, flags,
    instance and primitive exact, the three lods within their bound and exactly 0 or mips - 1 where the clamp decides, few hits undecided, more than 1 / 20 real;
    diffs = NULL is an array of zeros; the device forms and the composite call give the host form's bytes."""
    from sm64rt_legacy_renderer_amd import rt64
    case = cases[name]
    data = case["data"]
    w, h = case["render"]
    s = _open(rt64_lib, case)
    hip = ray_rule.Hip()
    try:
        textures = R.texture_table(data, _levels(rt64_lib, s, data))
        rays = ray_rule.random_rays(data, case["seed"], FC.RAYS, floor_instance=3)
        diffs = FC.random_diffs(case["seed"], rays)
        hits = rt64.trace_rays(rt64_lib, s.view, rays)
        got = rt64.footprint_hits(rt64_lib, s.view, rays, diffs, hits)
        bare = rt64.footprint_hits(rt64_lib, s.view, rays, None, hits)
        zeros = rt64.footprint_hits(rt64_lib, s.view, rays, np.zeros_like(diffs), hits)
        pixels = FC.all_pixels(case)
        crays, cdiffs = rt64.camera_rays(rt64_lib, s.view, pixels)
        chits = rt64.trace_rays(rt64_lib, s.view, crays)
        cgot = rt64.footprint_hits(rt64_lib, s.view, crays, cdiffs, chits)
        trays, thits, tgot = rt64.trace_pixel_footprints(rt64_lib, s.view, pixels)
        tonly = np.full_like(tgot, 7.0)          # rays = hits = NULL, pixels = NULL
        assert rt64_lib.TraceViewPixelFootprints(s.view, None, None, None, tonly.ctypes.data, len(pixels), 0) == 1, rt64_lib.last_error()
        d_rays, d_diffs, d_hits, d_rec = hip.upload(rays), hip.upload(diffs), hip.upload(hits), hip.alloc(got.nbytes)
        assert rt64_lib.FootprintViewRayHitsDevice(s.view, d_rays, d_diffs, d_hits, d_rec, len(rays), None) == 1, rt64_lib.last_error()
        dev = hip.download(d_rec, got)
        d_rec2, st = hip.alloc(got.nbytes), hip.stream()
        assert rt64_lib.FootprintViewRayHitsDevice(s.view, d_rays, None, d_hits, d_rec2, len(rays), st) == 1, rt64_lib.last_error()
        assert hip.h.hipStreamSynchronize(st) == 0
        dev_bare = hip.download(d_rec2, got)
    finally:
        hip.close()
        s.close()
    assert np.array_equal(_bits(bare), _bits(zeros)) and np.array_equal(_bits(dev), _bits(got)) and np.array_equal(_bits(dev_bare), _bits(bare))
    assert np.array_equal(_bits(trays), _bits(crays)) and np.array_equal(_bits(thits), _bits(chits))
    assert np.array_equal(_bits(tgot), _bits(cgot)) and np.array_equal(_bits(tonly), _bits(cgot))
    for tag, r, d, hh, g in ((" random", rays, diffs, hits, got), (" no diffs", rays, None, hits, bare), (" camera", crays, cdiffs, chits, cgot)):
        rule = _held_to_the_rule(name + tag, data, textures, r, d, hh, g)
        real = rule["kind"] == 2
        assert real.sum() > len(r) // 20 and np.array_equal(real, hh.view(np.int32)[:, 3] >= 0)
        assert rule["undecided"][real].mean() <= UNDECIDED_CAP, (name, tag)
    assert (bare[:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 13, 14]] == 0.0).all()          # F4: a zero differential -- gradients 0 (of either sign), lods 0, whatever the hit


@pytest.mark.parametrize("name", ["floor at a grazing angle", "floor at a grazing angle, POINT"])
def test_the_frames_texel_on_mip_mapped_textures(rt64_lib, cases, name):
    """3.  F9.  The floor at a grazing angle under generated chains, LINEAR and POINT: camera rays of pixels well inside one instance, walked as the frame walks, their
    footprints, and RT64_ShadeViewRayHits at lods = footprint.lod: colour against RT64_IMAGE_DIFFUSE (UNORM8) on every such pixel; on the floor, whose three maps
    are 64 x 64 under uvDetailScale 1, shadingNormal against RT64_IMAGE_SHADING_NORMAL (SNORM16, then RGBA16F) and specular against RT64_IMAGE_SHADING_SPECULAR
    (UNORM8, then RGBA16F) as well.  Allowed: half a storage step + the material rule's bound at that lod and, under LINEAR, + the lod's own bound (two levels
    differ by at most 1 in value, so a lod that is off by d moves the blend by at most d).  Under POINT a lod has no such slack, it selects a level: where the
    footprint rule calls that level undecided (the lod within its bound of a half-integer) the picture may show either of the two levels next to the lod, and
    the records shaded at each of them are accepted; everywhere else the level is the rule's (R.compare_levels) and the one record must match.  No compared pixel is
    degenerate or has a lod bound that is not finite (asserted); under POINT the pixels whose texel the material rule calls undecided are left out and counted.
    With lods = NULL -- level 0, what a host without this extension had -- the same pixels do not pass."""
    from sm64rt_legacy_renderer_amd import rt64
    case = cases[name]
    point = case["data"].shader_filter == 0
    data = case["data"]
    w, h = case["render"]
    s = _open(rt64_lib, case, lean_frames=0)
    try:
        levels = _levels(rt64_lib, s, data)
        assert len(levels[4]) == 7 and len(levels[5]) == 7 and len(levels[6]) == 7 and len(levels[1]) == 6
        hit = s.readback(rt64.IMAGE_PRIMARY_HIT)
        diffuse = s.readback(rt64.IMAGE_DIFFUSE)[..., :3].astype(np.float64)
        normal = s.readback(rt64.IMAGE_SHADING_NORMAL)[..., :3].astype(np.float64)
        specular = s.readback(rt64.IMAGE_SHADING_SPECULAR)[..., :3].astype(np.float64)
        inst = np.where(hit[..., 3] == 0xFFFFFFFF, -1, (hit[..., 3] >> 24).astype(np.int64))
        pad = np.pad(inst, 2, mode="edge")
        interior = inst >= 0
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                interior &= pad[2 + dy:2 + dy + h, 2 + dx:2 + dx + w] == inst
        ys, xs = np.nonzero(interior)
        pixels = np.stack([xs, ys], axis=1).astype(np.uint32)
        rays, diffs = rt64.camera_rays(rt64_lib, s.view, pixels)
        hits = rt64.trace_rays(rt64_lib, s.view, rays, rt64.RAY_FLAG_CULL_BACK_FACING)
        foot = rt64.footprint_hits(rt64_lib, s.view, rays, diffs, hits)
        lods = np.ascontiguousarray(foot[:, 4])
        frule = R.footprints(data, R.texture_table(data, levels), rays, diffs, hits)
        # the lods whose records are accepted: the footprint's own and, under POINT, the two levels next to the rule's lod
        tried = [lods] + ([np.floor(frule["lod"]["lod"]).astype(np.float32), np.ceil(frule["lod"]["lod"]).astype(np.float32)] if point else [])
        got = [rt64.shade_hits(rt64_lib, s.view, rays, hits, l) for l in tried]
        flat = rt64.shade_hits(rt64_lib, s.view, rays, hits)
    finally:
        s.close()
    assert np.array_equal(hits.view(np.int32)[:, 3], inst[ys, xs]) and len(set(inst[ys, xs].tolist())) == 2          # the sphere and the floor
    floor = hits.view(np.int32)[:, 3] == 1
    assert floor.sum() > 300 and (lods[floor] > 0.5).sum() > 100 and (lods[floor] > 1.5).sum() > 20          # minified: levels 1 and 2 are blended in (POINT: taken)
    assert np.array_equal(foot[floor, 5], lods[floor]) and np.array_equal(foot[floor, 6], lods[floor])         # one size, detail scale 1: one lod
    assert not frule["degenerate"].any() and np.isfinite(frule["lod"]["bound"]).all()                          # no pixel passes on an allowance that excludes nothing
    level_ok, level_compared = R.compare_levels(frule, foot)
    assert level_ok.all() and (level_compared > 1000) == point
    either = frule["lod"]["level_undecided"]
    assert not either.any() or point
    mrules = [M.materials(data, levels, rays, hits, l) for l in tried]
    lod_bound = np.zeros((len(rays), 1)) if point else frule["lod"]["bound"][:, None]
    assert point or (lod_bound[floor] <= R.DLOD).mean() > 0.9
    compared = ~np.any([m["undecided"] for m in mrules], axis=0) if point else np.ones(len(rays), dtype=bool)
    print("%s: %d interior pixels, %d left out (the material rule's texel undecided), %d with either of two levels accepted" % (name, len(rays), (~compared).sum(), (either & compared).sum()))
    assert compared.mean() >= 0.9
    misses = {}
    for what, image, cols, step, key, rows in (("colour", diffuse, slice(0, 3), HALF_UNORM8, "color", compared),
                                               ("shading normal", normal, slice(4, 7), HALF_SNORM16 + HALF_F16, "normal", floor & compared),
                                               ("specular", specular, slice(8, 11), HALF_UNORM8 + HALF_F16, "specular", floor & compared)):
        want = image[ys, xs]
        allowed = [step + m[key][1][:, :3] + lod_bound for m in mrules]
        inside = [(np.abs(g[:, cols].astype(np.float64) - want) <= a).all(axis=1) for g, a in zip(got, allowed)]
        ok = np.where(either, np.any(inside, axis=0), inside[0])          # the footprint's own lod must do wherever the level is decided
        d = np.abs(got[0][:, cols].astype(np.float64) - want)
        print("%s against the image at footprint.lod: max %.3e over %d pixels (allowed: %.3e + the rule's bound, at most %.1e, + the lod's, at most %.1e)"
              % (what, d[rows & ~either].max(), rows.sum(), step, mrules[0][key][1][rows].max(), lod_bound[rows].max()))
        assert ok[rows].all(), (what, np.nonzero(rows & ~ok)[0][:8].tolist())
        misses[what] = int((np.abs(flat[:, cols].astype(np.float64) - want)[rows] > allowed[0][rows]).any(axis=1).sum())
    print("at level 0 instead: %s pixels outside the same allowance" % misses)
    assert misses["colour"] > 50


def test_sizes_grid_stride_and_the_end_of_the_array(rt64_lib, cases):
    """4.  Counts 1, 63, 64, 65, 255, 256, 257 and RT_GRID_BLOCKS x RT_BLOCK + 65 (the grid-stride loop) of both kernels: each equals the prefix of one big host call,
    which crosses its staging chunks (2^18 records each) twice; guard words behind the last record stay untouched."""
    from sm64rt_legacy_renderer_amd import rt64
    case = cases["maps of other sizes, detail scales"]
    s = _open(rt64_lib, case)
    hip = ray_rule.Hip()
    try:
        rays = ray_rule.random_rays(case["data"], 29, 2000, floor_instance=3)
        diffs = FC.random_diffs(29, rays)
        hits = rt64.trace_rays(rt64_lib, s.view, rays)
        big = 2048 * 256 + 65
        reps = -(-(big + 300) // len(rays))
        rng = np.random.default_rng(5)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(reps - 1)])          # later repetitions shuffled: waves mix instances
        many = [np.ascontiguousarray(a[order]) for a in (rays, diffs, hits)]
        n = len(order)
        whole = _bits(rt64.footprint_hits(rt64_lib, s.view, *many))
        first = _bits(rt64.footprint_hits(rt64_lib, s.view, rays, diffs, hits))
        for r in range(reps):
            rows = slice(r * len(rays), (r + 1) * len(rays))
            assert np.array_equal(whole[rows], first[order[rows]]), r
        pixels = rng.integers(0, 300, size=(n, 2)).astype(np.uint32)
        prays, pdiffs = rt64.camera_rays(rt64_lib, s.view, pixels)
        d_in = [hip.upload(a) for a in many]
        d_pix = hip.upload(pixels)
        guard = np.full((n, 16), 0xABABABAB, dtype=np.uint32)
        for count in (1, 63, 64, 65, 255, 256, 257, big):
            d_guard = hip.upload(guard[:count + 258])
            assert rt64_lib.FootprintViewRayHitsDevice(s.view, d_in[0], d_in[1], d_in[2], d_guard, count, None) == 1, rt64_lib.last_error()
            out = hip.download(d_guard, guard[:count + 258])
            assert np.array_equal(out[:count], whole[:count]) and (out[count:] == 0xABABABAB).all(), count
            d_g1, d_g2 = hip.upload(guard[:count + 258, :8]), hip.upload(guard[:count + 258])
            assert rt64_lib.GenerateViewCameraRaysDevice(s.view, d_pix, d_g1, d_g2, count, None) == 1, rt64_lib.last_error()
            o1, o2 = hip.download(d_g1, guard[:count + 258, :8]), hip.download(d_g2, guard[:count + 258])
            assert np.array_equal(o1[:count], _bits(prays)[:count]) and (o1[count:] == 0xABABABAB).all(), count
            assert np.array_equal(o2[:count], _bits(pdiffs)[:count]) and (o2[count:] == 0xABABABAB).all(), count
            for p in (d_guard, d_g1, d_g2):
                assert hip.h.hipFree(p) == 0
                hip.ptrs.remove(p)
    finally:
        hip.close()
        s.close()


def test_a_frame_without_ray_traced_instances_has_no_camera_rays(rt64_lib, cases):
    """F10: a frame that traced no instance keeps no frame parameters, so the generate calls are refused with a message that says so; the footprint call answers
    (every hit index is out of range: BAD_HIT records)."""
    import copy
    from sm64rt_legacy_renderer_amd import rt64
    case = dict(cases["sample, generated mips"])
    data = copy.copy(case["data"])
    data.meshes = [copy.copy(m) for m in data.meshes]
    for m in data.meshes:
        m.flags = 0                                   # raster only: nothing is ray traced
    case["data"] = data
    s = _open(rt64_lib, case)
    try:
        out = np.full((4, 8), 0xABABABAB, dtype=np.uint32)
        for call, fn in ((lambda: rt64_lib.GenerateViewCameraRays(s.view, None, out.ctypes.data, None, 4), "RT64_GenerateViewCameraRays"),
                         (lambda: rt64_lib.TraceViewPixelFootprints(s.view, None, out.ctypes.data, None, np.empty((4, 16), dtype=np.float32).ctypes.data, 4, 0), "RT64_TraceViewPixelFootprints")):
            assert call() == 0 and fn + ":" in rt64_lib.last_error() and "no instance" in rt64_lib.last_error(), rt64_lib.last_error()
        assert (out == 0xABABABAB).all()
        rays = np.zeros((4, 8), dtype=np.float32); rays[:, 6] = -1.0; rays[:, 7] = 10.0
        hits = np.zeros((4, 8), dtype=np.float32)      # instance 0, primitive 0: out of range here
        rec = rt64.footprint_hits(rt64_lib, s.view, rays, None, hits)
        assert (_bits(rec)[:, 7] == R.BAD_HIT).all() and (_bits(rec)[:, 11] == 0xFFFFFFFF).all()
    finally:
        s.close()


def test_misses_bad_hits_and_refusals(rt64_lib, cases):
    """5.  F4: misses give the miss record, out-of-range instances and primitives BAD_HIT records, garbage t, u, v a record and no fault.  F10: every refusal returns 0
    with a message that names the function; count = 0 succeeds and touches nothing; more rays than pixels with pixels = NULL, unknown flags and misaligned device
    arrays are refused; after RT64_DestroyTexture of a texture the frame used the footprint calls are refused while the camera rays still come, until the next draw."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    case = dict(cases["sample, generated mips"], frames=0)
    data = case["data"]
    w, h = case["render"]
    s = _open(rt64_lib, case)
    hip = ray_rule.Hip()
    R_ = rt64_lib
    try:
        rays = ray_rule.random_rays(data, 31, 600, floor_instance=3)
        diffs = FC.random_diffs(31, rays)
        hits = np.zeros_like(rays); hits.view(np.int32)[:, 3] = -1
        rec = np.full((len(rays), 16), 0xABABABAB, dtype=np.uint32)
        ray_out = np.full((len(rays), 8), 0xABABABAB, dtype=np.uint32)

        def refused(word, fn, call):
            ok = call()
            assert ok == 0 and fn + ":" in R_.last_error() and word in R_.last_error(), (ok, R_.last_error())
        foot = lambda n=len(rays), r=rays, d=diffs, hh=None, o=rec: R_.FootprintViewRayHits(s.view, r.ctypes.data if r is not None else None, d.ctypes.data if d is not None else None,
                                                                                           (hits if hh is None else hh).ctypes.data, o.ctypes.data if o is not None else None, n)
        gen = lambda n=len(rays), o=ray_out: R_.GenerateViewCameraRays(s.view, None, o.ctypes.data if o is not None else None, None, n)
        comp = lambda n=len(rays), flags=0, o=rec: R_.TraceViewPixelFootprints(s.view, None, None, None, o.ctypes.data if o is not None else None, n, flags)
        refused("draw", "RT64_FootprintViewRayHits", foot)                          # before the first frame
        refused("draw", "RT64_GenerateViewCameraRays", gen)
        refused("draw", "RT64_TraceViewPixelFootprints", comp)
        assert (rec == 0xABABABAB).all() and (ray_out == 0xABABABAB).all()
        s.draw()
        textures = R.texture_table(data, _levels(R_, s, data))
        hits = rt64.trace_rays(R_, s.view, rays)
        hi = hits.view(np.int32)
        real, miss = np.nonzero(hi[:, 3] >= 0)[0], np.nonzero(hi[:, 3] < 0)[0]
        assert len(real) > 30 and len(miss) > 30
        edited = hits.copy(); ei = edited.view(np.int32)
        rt = R.S.raytraced_instances(data)
        ei[real[0], 3] = len(rt)                                                          # just past the end, nothing wilder
        ei[real[1], 4] = len(data.meshes[data.instances[rt[int(hi[real[1], 3])]].mesh].indices) // 3
        ei[real[2], 3] = 0x7FFFFFFF; ei[real[3], 4] = -1                                  # ... and the wildest
        got = rt64.footprint_hits(R_, s.view, rays, diffs, edited)
        rule = _held_to_the_rule("edited hits", data, textures, rays, diffs, edited, got, say=False)
        gi = _bits(got)
        assert (rule["kind"][real[:4]] == 1).all() and (rule["kind"][real[4:]] == 2).all()
        for rows, flags in ((miss, 0), (real[:4], R.BAD_HIT)):
            assert (gi[rows, 7] == flags).all() and (gi[rows, 11] == 0xFFFFFFFF).all() and (gi[rows, 15] == 0xFFFFFFFF).all()
            assert not gi[rows][:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 13, 14]].any()
        # garbage t and barycentrics, garbage differentials: a record comes back for each, flags VALID, lods inside their range (F8), and the call succeeds
        wild = hits[real[4:]].copy(); wr = rays[real[4:]]; wd = diffs[real[4:]].copy()
        vals = np.array([1e30, -1e30, np.inf, -np.inf, np.nan, 3.0e9, -7.5, 1e-40], dtype=np.float32)
        wild[:, 0] = vals[np.arange(len(wild)) % 8]; wild[:, 1] = vals[(np.arange(len(wild)) // 8) % 8]
        wd[::3, 8:11] = vals[np.arange(len(wd[::3])) % 8][:, None]; wd[1::3, 0:3] = vals[(np.arange(len(wd[1::3])) + 3) % 8][:, None]
        gw = rt64.footprint_hits(R_, s.view, wr, wd, wild)
        assert (_bits(gw)[:, 7] & R.VALID).all() and np.array_equal(_bits(gw)[:, 11], _bits(wild)[:, 3]) and np.array_equal(_bits(gw)[:, 15], _bits(wild)[:, 4])
        assert np.isfinite(gw[:, 4:7]).all() and (gw[:, 4:7] >= 0.0).all() and (gw[:, 4:7] <= 6.0).all()
        # count = 0 succeeds and touches nothing; NULL arrays, a NULL view, unknown flags, too many pixels and misaligned device arrays are refused
        rec[:] = 0xABABABAB
        assert foot(0) == 1 and gen(0) == 1 and comp(0) == 1
        assert (rec == 0xABABABAB).all() and (ray_out == 0xABABABAB).all()
        refused("NULL", "RT64_FootprintViewRayHits", lambda: foot(4, r=None))
        refused("NULL", "RT64_FootprintViewRayHits", lambda: foot(4, o=None))
        refused("NULL", "RT64_GenerateViewCameraRays", lambda: gen(4, o=None))
        refused("NULL", "RT64_TraceViewPixelFootprints", lambda: comp(4, o=None))
        refused("NULL view", "RT64_FootprintViewRayHits", lambda: R_.FootprintViewRayHits(None, rays.ctypes.data, None, hits.ctypes.data, rec.ctypes.data, 4))
        refused("unknown flags", "RT64_TraceViewPixelFootprints", lambda: comp(4, flags=rt64.RAY_FLAG_ACCEPT_FIRST_HIT))
        refused("pixels", "RT64_GenerateViewCameraRays", lambda: R_.GenerateViewCameraRays(s.view, None, np.empty((w * h + 1, 8), dtype=np.float32).ctypes.data, None, w * h + 1))
        big = np.empty((w * h, 8), dtype=np.float32)
        assert R_.GenerateViewCameraRays(s.view, None, big.ctypes.data, None, w * h) == 1
        assert R_.TraceViewPixelFootprints(s.view, None, None, None, rec.ctypes.data, 4, rt64.RAY_FLAG_CULL_BACK_FACING) == 1
        d_rays, d_diffs, d_hits, d_rec, d_pix = hip.upload(rays), hip.upload(diffs), hip.upload(hits), hip.alloc(rec.nbytes), hip.upload(np.zeros((len(rays), 2), dtype=np.uint32))
        dev = "RT64_FootprintViewRayHitsDevice"
        for a, b, c, d in ((d_rays + 4, d_diffs, d_hits, d_rec), (d_rays, d_diffs + 8, d_hits, d_rec), (d_rays, d_diffs, d_hits + 4, d_rec), (d_rays, d_diffs, d_hits, d_rec + 8)):
            refused("aligned", dev, lambda: R_.FootprintViewRayHitsDevice(s.view, a, b, c, d, 4, None))
        gdev = "RT64_GenerateViewCameraRaysDevice"
        refused("aligned", gdev, lambda: R_.GenerateViewCameraRaysDevice(s.view, d_pix + 4, d_rays, d_diffs, 4, None))
        refused("aligned", gdev, lambda: R_.GenerateViewCameraRaysDevice(s.view, d_pix, d_rays + 8, d_diffs, 4, None))
        refused("aligned", gdev, lambda: R_.GenerateViewCameraRaysDevice(s.view, d_pix, d_rays, d_diffs + 4, 4, None))
        assert R_.GenerateViewCameraRaysDevice(s.view, d_pix + 8, d_rec, None, 4, None) == 1          # pixels need 8-byte alignment only
        # RT64_SetMesh on a mesh the frame traced: the footprints are refused, the camera rays are not (they read no mesh)
        m = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], m.vertices, m.indices)
        refused("RT64_SetMesh", "RT64_FootprintViewRayHits", lambda: foot(4))
        refused("RT64_SetMesh", "RT64_TraceViewPixelFootprints", lambda: comp(4))
        assert gen(4) == 1
        s.draw()
        assert np.array_equal(_bits(rt64.footprint_hits(R_, s.view, rays, diffs, edited)), gi)
        # RT64_DestroyTexture of a texture the frame's table holds (a copy of the floor's specular map on an extra instance, which goes first)
        t = data.textures[6]
        td = rt64.TEXTURE_DESC(); buf, pitch = t.upload_buffer()
        td.bytes = buf.ctypes.data; td.byteCount = buf.nbytes; td.format = t.format; td.width, td.height, td.rowPitch = t.width, t.height, pitch
        th = R_.CreateTexture(s.device, td)
        assert th, R_.last_error()
        s.textures.append(th)
        far = data.instances[1]
        tr = np.array(far.transform, dtype=np.float32).copy(); tr[3, 0] -= np.float32(3.0)
        ih = R_.CreateInstance(s.scene); s.instances.append(ih)
        s.set_instance(len(s.instances) - 1, sample_scene.InstanceData("extra", far.mesh, tr, tr, far.diffuse, None, len(s.textures) - 1, far.material))
        s.draw()
        before = rt64.camera_rays(R_, s.view, None, count=64)
        assert rt64.footprint_hits(R_, s.view, rays, diffs, rt64.trace_rays(R_, s.view, rays)) is not None
        R_.DestroyInstance(ih); s.instances.pop()
        R_.DestroyTexture(th); s.textures.pop()
        refused("texture", "RT64_FootprintViewRayHits", lambda: foot(4))
        refused("texture", dev, lambda: R_.FootprintViewRayHitsDevice(s.view, d_rays, d_diffs, d_hits, d_rec, 4, None))
        refused("texture", "RT64_TraceViewPixelFootprints", lambda: comp(4))
        after = rt64.camera_rays(R_, s.view, None, count=64)          # the generate calls read no texture
        assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(_bits(after[1]), _bits(before[1]))
        s.draw()
        assert np.array_equal(_bits(rt64.footprint_hits(R_, s.view, rays, diffs, edited)), gi)
    finally:
        hip.close()
        s.close()


def test_footprint_queries_between_frames_leave_the_frames_alone(rt64_lib, sample_data):
    """6.  A GI + denoiser sequence with camera-ray, footprint and composite calls between its frames -- host arrays, and device arrays on a caller stream -- renders
    byte-identical images to the same sequence without them (frames enqueued: sync_present = 0)."""
    import copy
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    rays = ray_rule.random_rays(sample_data, 51, 2000, floor_instance=3)
    diffs = FC.random_diffs(51, rays)
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
            d_rays, d_diffs, d_hits, d_rec = hip.upload(rays), hip.upload(diffs), hip.alloc(rays.nbytes), hip.alloc(len(rays) * 64)
            d_cam, d_cdiff = hip.alloc(96 * 64 * 32), hip.alloc(96 * 64 * 64)
            for f in range(3):
                v = np.array(sample_data.view, dtype=np.float32).copy(); v[3, 0] += np.float32(0.05 * f)
                data.view = v
                s.draw()
                hits = rt64.trace_rays(rt64_lib, s.view, rays)
                if query:
                    rt64.footprint_hits(rt64_lib, s.view, rays, diffs, hits)
                    rt64.trace_pixel_footprints(rt64_lib, s.view, None, count=96 * 64, flags=rt64.RAY_FLAG_CULL_BACK_FACING)
                    assert hip.h.hipMemcpy(d_hits, hits.ctypes.data, hits.nbytes, 1) == 0
                    assert rt64_lib.GenerateViewCameraRaysDevice(s.view, None, d_cam, d_cdiff, 96 * 64, st) == 1
                    assert rt64_lib.FootprintViewRayHitsDevice(s.view, d_rays, d_diffs, d_hits, d_rec, len(rays), st) == 1
                out.append([s.readback(k).copy() for k in images] + [hits])
            return out
        finally:
            hip.close()
            s.close()
    a, b = run(False), run(True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert x.tobytes() == y.tobytes()
