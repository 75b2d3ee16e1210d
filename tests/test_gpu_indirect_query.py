"""The indirect light of a point as a frame's pixel samples it (RT64_GenerateViewPointGIRays, RT64_ComposeViewGIRays, RT64_TraceViewPointsIndirect,
RT64_TraceViewRayIndirect, include/rt64_indirect.h; rules Y1-Y12 in DESIGN.md 4) on the GPU.

The scenes are the 88 x 72 sessions of tests/gi_cases.py.  The points are the ones a frame stored (SHADING_POSITION, SHADING_NORMAL, INSTANCE_ID of its surface pixels), keyed
(x, y, frameCount): the records are held to tests/gi_rule.py, the float64 statement of the frame's GI pass, inside the rule's own bound (1), to the frame's INDIRECT_LIGHT_RAW
and GI_MOMENTS inside twice that bound (2) and against every wrong reading of the rule its cases were built to catch (3); then to themselves: keys (4), the chain against its
links (5), the hit form (6), overrides (7), forms, sizes and the ends of the arrays (8), refusals and counters (9).  The rule runs once per (case, frame): the runs share it.

One run's lines of (2) are committed as profiles/indirect_rule_deviation.txt.
"""
import ctypes as C

import numpy as np
import pytest

import gi_cases as GC
import gi_rule as G
import light_rule as L
import ray_rule
from light_rule import F

pytestmark = pytest.mark.gpu

W, H = GC.W, GC.H
CASES = ("opaque-3", "self-lit", "layers", "background", "sky-strength", "two-bounce-opaque", "two-bounce-layers")
CULL = ray_rule.CULL_BACK_FACING
GUARD = 0xABABABAB
_runs, _rules = {}, {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rec(records):
    from sm64rt_legacy_renderer_amd import rt64
    return np.ascontiguousarray(records).view(rt64.POINT_INDIRECT_DTYPE).reshape(-1)


def _smp(samples):
    from sm64rt_legacy_renderer_amd import rt64
    a = np.ascontiguousarray(samples)
    return a.view(rt64.GI_SAMPLE_DTYPE).reshape(a.shape[:-1])


def _open(rt64_lib, case, options=None):
    """The session of gi_cases.gpu_session, left open: nothing drawn yet."""
    from sm64rt_legacy_renderer_amd import sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, case["data_at"](0), W, H, hip_device=0)
    try:
        s.set_view_description(denoiser=False, **case["view"])
        assert s.option("max_reflections", 0) and s.option("gi_bounces", case["bounces"])
        for key, v in (options or {}).items():
            assert s.option(key, v), key
    except Exception:
        s.close()
        raise
    return s


def _images(s, case):
    from sm64rt_legacy_renderer_amd import rt64
    img = {key: s.readback(getattr(rt64, "IMAGE_" + name)) for key, name in GC.GPU_IMAGES.items()}
    img["background"] = s.readback(rt64.IMAGE_BACKGROUND) if case["background"] else None
    return img


def _points(img, mask=None):
    """RT64_GI_POINTs of the frame's surface pixels (INSTANCE_ID >= 0; `mask` narrows them), their keys' (x, y) and their pixel numbers."""
    surface = np.asarray(img["id"]) >= 0
    if mask is not None:
        surface = surface & mask
    ys, xs = np.nonzero(surface)
    p = np.zeros((len(xs), 8), dtype=np.float32)
    p[:, 0:3] = np.asarray(img["position"])[ys, xs, :3]
    p[:, 4:7] = np.asarray(img["normal"])[ys, xs, :3].astype(np.float32)
    p.view(np.int32)[:, 7] = np.asarray(img["id"])[ys, xs]
    return p, xs.astype(np.uint32), ys.astype(np.uint32)


def _keys(xs, ys, frame):
    k = np.zeros((len(xs), 4), dtype=np.uint32)
    k[:, 0], k[:, 1], k[:, 2] = xs, ys, frame
    return k


def _run(rt64_lib, sample_data, name, cache):
    """One session of a case with the LDS scene cache on or off: per compared frame the stored images, the points of its surface pixels and their records."""
    from sm64rt_legacy_renderer_amd import rt64
    if (name, cache) in _runs:
        return _runs[name, cache]
    case = GC.make_case(sample_data, name)
    out = {}
    s = _open(rt64_lib, case, {"lds_cache": cache})
    try:
        for f in range(case["frames"]):
            s.data = case["data_at"](f)
            s.draw()
            if f not in case["compared"]:
                continue
            img = _images(s, case)
            pts, xs, ys = _points(img)
            records = rt64.sample_indirect(rt64_lib, s.view, pts, _keys(xs, ys, f))
            out[f] = dict(img=img, points=pts, xs=xs, ys=ys, records=records)
    finally:
        s.close()
    _runs[name, cache] = (case, out)
    return case, out


def _rule(case, f, img, mutate=None):
    """gi_rule on a frame's stored inputs, once per (case, frame, mutation) and input bytes."""
    known = [r for i, r in _rules.setdefault((case["name"], f, mutate), []) if GC.inputs_equal(i, img)]
    if not known:
        _rules[case["name"], f, mutate].append(({k: img[k] for k in GC.INPUTS}, GC.run_rule(case, f, img, mutate=mutate)))
        known = [_rules[case["name"], f, mutate][-1][1]]
    return known[0]


def _as_images(run, base_raw, base_moments):
    """The records as the two images gi_rule.compare takes: the queried pixels from the records, the others (not queried) from `base_*`."""
    r = _rec(run["records"])
    raw = np.array(base_raw, dtype=np.float64); mom = np.array(base_moments, dtype=np.float64)
    raw[run["ys"], run["xs"], 0:3] = r["indirect"]; raw[run["ys"], run["xs"], 3] = r["samples"]
    mom[run["ys"], run["xs"]] = r["moments"]
    return raw, mom


# ---- 1. points stored by a frame, held to gi_rule ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("name", CASES)
def test_records_of_stored_points_lie_within_the_rule(rt64_lib, sample_data, name, cache):
    """1.  indirect and moments within gi_rule.indirect's bound at every decided pixel (the bound holds half an f16 step, which a float32 record does not use); samples,
    flags and instance exact; undecided pixels under the cap; the case's shares of hit, miss, lit, shadowed, two-layer and sky rays present in the rule's own counts."""
    from sm64rt_legacy_renderer_amd import rt64
    case, out = _run(rt64_lib, sample_data, name, cache)
    total = {}
    for f in case["compared"]:
        run = out[f]
        rule = _rule(case, f, run["img"])
        r = _rec(run["records"])
        assert len(r) == int(rule["surface"].sum()) > 1000
        assert (r["flags"] == rt64.INDIRECT_VALID).all() and (r["samples"] == np.float32(case["view"]["gi_samples"])).all()
        assert np.array_equal(r["instance"], np.asarray(run["img"]["id"])[run["ys"], run["xs"]])
        assert (r["rays"] >= case["view"]["gi_samples"]).all() and (r["rays"] <= case["view"]["gi_samples"] * case["bounces"]).all()
        raw, mom = _as_images(run, rule["value"], rule["moments"])
        worst, mean, bad = G.compare(raw, mom, rule)
        und = int((~rule["decided"]).sum())
        print("indirect_rule %-18s lds_cache=%d frame %d ratio=%.6f mean=%.6f points=%d undecided=%d counts %s" % (name, cache, f, worst, mean, len(r), und, rule["info"]["counts"]))
        assert int(bad.sum()) == 0 and worst < 1.0, (name, f, worst, int(bad.sum()))
        assert und <= int(GC.UNDECIDED_CAP * len(r)), (name, f, und)
        for k, v in rule["info"]["counts"].items():
            total[k] = total.get(k, 0) + v
    for k, need in GC.SHARES[name].items():
        assert total.get(k, 0) >= need and total.get(k, 0) > 0, (name, k, total.get(k, 0), need)


# ---- 2. agreement with the frame --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("name", CASES)
def test_records_agree_with_the_frame(rt64_lib, sample_data, name, cache):
    """2.  float16(indirect) against INDIRECT_LIGHT_RAW.rgb and moments against GI_MOMENTS: both sides lie inside the rule, so they differ by less than twice its bound at
    every decided pixel.  The count of bit-equal pixels and the largest ratio are printed (profiles/indirect_rule_deviation.txt)."""
    case, out = _run(rt64_lib, sample_data, name, cache)
    for f in case["compared"]:
        run = out[f]
        rule = _rule(case, f, run["img"])
        r = _rec(run["records"])
        ys, xs = run["ys"], run["xs"]
        frame_rgb = np.asarray(run["img"]["raw"])[ys, xs, :3]
        frame_m = np.asarray(run["img"]["moments"])[ys, xs]
        mine = r["indirect"].astype(np.float16)
        dev = np.concatenate([np.abs(mine.astype(np.float64) - frame_rgb.astype(np.float64)), np.abs(r["moments"].astype(np.float64) - frame_m.astype(np.float64))], axis=-1)
        b = 2.0 * np.concatenate([rule["bound"][ys, xs, :3], rule["moments_bound"][ys, xs]], axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(dev == 0.0, 0.0, dev / b).max(axis=-1)
        ok = rule["decided"][ys, xs]
        equal_rgb = (mine.view(np.uint16) == np.asarray(frame_rgb, dtype=np.float16).view(np.uint16)).all(axis=-1)
        equal_m = (_bits(r["moments"]) == _bits(np.asarray(frame_m, dtype=np.float32))).all(axis=-1)
        print("indirect_frame %-18s lds_cache=%d frame %d points=%d bit-equal rgb %d moments %d  largest |record - frame| / (2 x bound) %.6f" %
              (name, cache, f, len(r), int(equal_rgb.sum()), int(equal_m.sum()), float(ratio[ok].max())))
        assert (np.asarray(run["img"]["raw"])[ys, xs, 3] == r["samples"]).all()
        assert (ratio[ok] < 1.0).all(), (name, f, float(ratio[ok].max()))


# ---- 3. wrong readings are seen -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutation", [m for m in G.MUTATIONS if GC.MUTATION_CASE[m] in CASES])
def test_a_wrong_reading_puts_the_records_outside_its_bound(rt64_lib, sample_data, mutation):
    """3.  The mutated rule must put the RECORDS outside its bound on more points than it leaves undecided."""
    name = GC.MUTATION_CASE[mutation]
    case, out = _run(rt64_lib, sample_data, name, 1)
    outside = undecided = 0
    for f in case["compared"]:
        run = out[f]
        wrong = _rule(case, f, run["img"], mutate=mutation)
        raw, mom = _as_images(run, wrong["value"], wrong["moments"])
        _, _, bad = G.compare(raw, mom, wrong)
        outside += int(bad.sum()); undecided += int((~wrong["decided"]).sum())
    print("    mutation %-26s on %-18s %5d records outside its bound, %d undecided" % (mutation, name, outside, undecided))
    assert outside > undecided, (mutation, outside, undecided)


# ---- 4. keys ------------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_keys(rt64_lib, sample_data):
    """4.  Explicit keys (x, y, frameCount) equal keys = NULL bit for bit; a key with frame f equals the record of a twin session drawn up to frame f; shuffled points give
    the same records permuted; keys outside the frame are legal (only x % 64, y % 64 and x + y * width are formed, and no shader of these scenes has the noise option, so
    a key 64 texels further on gives the same record)."""
    from sm64rt_legacy_renderer_amd import rt64
    case = GC.make_case(sample_data, "opaque-3")
    s = _open(rt64_lib, case)
    try:
        s.draw()
        img = _images(s, case)
        surface = np.asarray(img["id"]).reshape(-1) >= 0
        # every pixel of the frame row by row: the others stand for "no point"
        every = np.zeros((W * H, 8), dtype=np.float32)
        every[:, 0:3] = np.asarray(img["position"]).reshape(-1, 4)[:, :3]; every[:, 4:7] = np.asarray(img["normal"]).reshape(-1, 4)[:, :3].astype(np.float32)
        every.view(np.int32)[:, 7] = np.asarray(img["id"]).reshape(-1)
        every.view(np.uint32)[~surface, 3] = rt64.GI_POINT_NONE
        by_place = _bits(rt64.sample_indirect(rt64_lib, s.view, every))
        pts, xs, ys = _points(img)
        keyed = {f: _bits(rt64.sample_indirect(rt64_lib, s.view, pts, _keys(xs, ys, f))) for f in (0, 1, 3)}
        assert np.array_equal(by_place[surface], keyed[0])
        none = _rec(by_place[~surface])
        assert not by_place[~surface][:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]].any() and (none["instance"] == -1).all() and (~surface).sum() > 500
        assert not np.array_equal(keyed[0], keyed[1]) and not np.array_equal(keyed[1], keyed[3])
        order = np.random.default_rng(11).permutation(len(pts))
        shuffled = _bits(rt64.sample_indirect(rt64_lib, s.view, np.ascontiguousarray(pts[order]), np.ascontiguousarray(_keys(xs, ys, 1)[order])))
        assert np.array_equal(shuffled, keyed[1][order])
        far = _keys(xs + 64 * 1000, ys + 64 * 1000000, 1)          # (y * width wraps in 32 bits)
        assert np.array_equal(_bits(rt64.sample_indirect(rt64_lib, s.view, pts, far)), keyed[1])
    finally:
        s.close()
    s = _open(rt64_lib, case)
    try:
        drawn = 0
        for f in (1, 3):
            while drawn < f + 1:
                s.draw(); drawn += 1
            twin = _bits(rt64.sample_indirect(rt64_lib, s.view, pts, _keys(xs, ys, f)))
            assert np.array_equal(twin, keyed[f]), f
            place = np.zeros((W * H, 8), dtype=np.float32); place.view(np.uint32)[:, 3] = rt64.GI_POINT_NONE
            place[ys * W + xs] = pts
            assert np.array_equal(_bits(rt64.sample_indirect(rt64_lib, s.view, place))[ys * W + xs], keyed[f]), f          # keys = NULL: the twin's own frame count
    finally:
        s.close()


# ---- 5. the chain is its parts --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["layers", "two-bounce-layers", "two-bounce-opaque"])
def test_the_chain_is_its_parts(rt64_lib, sample_data, name):
    """5.  gi_rays -> RT64_TraceViewRayLayers -> shade_gi_rays equals the composite's optional `samples` output bit for bit, for one and two bounces; `indirect` and `moments`
    follow from `samples` within the bounds of the rule's own lerp / rcp / add arithmetic (light_rule.F)."""
    from sm64rt_legacy_renderer_amd import rt64
    case = GC.make_case(sample_data, name)
    S = case["view"]["gi_samples"]
    s = _open(rt64_lib, case)
    try:
        s.draw(); s.draw()
        pts, xs, ys = _points(_images(s, case))
        keys = _keys(xs, ys, 1)
        records, samples = rt64.sample_indirect(rt64_lib, s.view, pts, keys, gi_samples=S, samples=True)
        assert samples.shape == (S, len(pts), 16)
        assert np.array_equal(_bits(records), _bits(rt64.sample_indirect(rt64_lib, s.view, pts, keys)))
        for k in range(S):
            slot = S - k
            rays = rt64.gi_rays(rt64_lib, s.view, pts, slot, keys)
            assert np.array_equal(rays[:, 0:3], pts[:, 0:3]) and (rays[:, 3] == np.float32(0.1)).all() and (rays[:, 7] == np.float32(100000.0)).all()
            hits, _ = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 16, flags=CULL)
            incoming = None
            if case["bounces"] == 2:
                first = _smp(rt64.shade_gi_rays(rt64_lib, s.view, rays, hits, keys))
                on = (first["flags"] & rt64.GI_SAMPLE_SURFACE) != 0
                assert on.sum() > 500 and (~on).sum() > 500
                second = np.zeros((len(pts), 8), dtype=np.float32)
                second[:, 0:3] = first["position"]; second[:, 4:7] = first["normal"]; second.view(np.int32)[:, 7] = first["instance"]
                second.view(np.uint32)[~on, 3] = rt64.GI_POINT_NONE
                rays2 = rt64.gi_rays(rt64_lib, s.view, second, slot, keys, second_bounce=True)
                assert not rays2[~on].any()
                hits2, _ = rt64.trace_view_ray_layers(rt64_lib, s.view, rays2, 16, flags=CULL)
                incoming = np.ascontiguousarray(rt64.shade_gi_rays(rt64_lib, s.view, rays2, hits2, keys)[:, 0:3])
            parts = rt64.shade_gi_rays(rt64_lib, s.view, rays, hits, keys, incoming)
            assert np.array_equal(_bits(parts), _bits(samples[k])), (name, slot)
    finally:
        s.close()
    sm, r = _smp(samples), _rec(records)
    assert ((sm["flags"] & rt64.GI_SAMPLE_VALID) != 0).all()
    acc = [F(np.zeros(len(pts))) for _ in range(3)]
    sum_l, sum_l2 = F(np.zeros(len(pts))), F(np.zeros(len(pts)))
    for k in range(S):
        rad = [F(sm["radiance"][k][:, c].astype(np.float64)) for c in range(3)]
        inv = L.rcp(F(np.full(len(pts), float(k + 1))))
        acc = [L.lerp(acc[c], rad[c], inv) for c in range(3)]
        lum = L.add(L.add(L.mul(rad[0], G.LUMA[0]), L.mul(rad[1], G.LUMA[1])), L.mul(rad[2], G.LUMA[2]))
        sum_l = L.add(sum_l, lum); sum_l2 = L.add(sum_l2, L.mul(lum, lum))
    m = [L.div(sum_l, float(S)), L.div(sum_l2, float(S))]
    for c in range(3):
        assert (np.abs(r["indirect"][:, c].astype(np.float64) - acc[c].v) <= acc[c].e + L.U * np.abs(acc[c].v)).all(), (name, c)
    for c in range(2):
        assert (np.abs(r["moments"][:, c].astype(np.float64) - m[c].v) <= m[c].e + 2.0 * L.U * np.abs(m[c].v)).all(), (name, c)


# ---- 6. the hit form --------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_hit_form(rt64_lib, sample_data):
    """6.  trace_indirect on a frame's camera rays against sample_indirect fed the positions of RT64_ResolveViewRayHits and the mapped normals of RT64_ShadeViewRayHits (flipped
    on a back face, as that call returns them): bit for bit; misses give zero records with instance -1."""
    from sm64rt_legacy_renderer_amd import rt64
    case = GC.make_case(sample_data, "layers")
    s = _open(rt64_lib, case)
    try:
        s.draw()
        rays = rt64.camera_rays(rt64_lib, s.view, None, W * H, differentials=False)
        hits, records = rt64.trace_indirect(rt64_lib, s.view, rays)
        assert np.array_equal(_bits(hits)[:, :5], _bits(rt64.trace_rays_alpha(rt64_lib, s.view, rays))[:, :5])
        surf = rt64.resolve_hits(rt64_lib, s.view, rays, hits)
        mat = rt64.shade_hits(rt64_lib, s.view, rays, hits)
        inst = hits.view(np.int32)[:, 3]
        real = inst >= 0
        pts = np.zeros((W * H, 8), dtype=np.float32)
        pts[:, 0:3] = surf[:, 0:3]; pts[:, 4:7] = mat[:, 4:7]; pts.view(np.int32)[:, 7] = inst
        pts.view(np.uint32)[~real, 3] = rt64.GI_POINT_NONE
        assert np.array_equal(_bits(rt64.sample_indirect(rt64_lib, s.view, pts)), _bits(records))
        r = _rec(records)
        assert real.sum() > 1000 and (~real).sum() > 500
        assert (r["instance"][~real] == -1).all() and not _bits(records)[~real][:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]].any()
        assert (r["flags"][real] == rt64.INDIRECT_VALID).all() and np.array_equal(r["instance"][real], inst[real])
        h2, culled = rt64.trace_indirect(rt64_lib, s.view, rays, flags=CULL)
        assert np.array_equal(_bits(h2)[:, :5], _bits(rt64.trace_rays_alpha(rt64_lib, s.view, rays, None, CULL))[:, :5])
    finally:
        s.close()


# ---- 7. overrides -------------------------------------------------------------------------------------------------------------------------------------------------------------------

OVERRIDES = [("opaque-3", dict(gi_samples=0)), ("opaque-3", dict(gi_samples=1)), ("opaque-3", dict(gi_samples=3)), ("opaque-3", dict(gi_samples=4)), ("opaque-3", dict(gi_samples=64)),
             ("opaque-3", dict(di_samples=0)), ("opaque-3", dict(di_samples=2)), ("layers", dict(gi_bounces=2))]


@pytest.mark.parametrize("name,over", OVERRIDES, ids=["%s-%s" % (n, "-".join("%s-%d" % kv for kv in o.items())) for n, o in OVERRIDES])
def test_overrides_follow_the_rule_with_the_fields_changed(rt64_lib, sample_data, name, over):
    """7.  giSamples 0 (I1), 1, 3 (the rounding reciprocal), 4 and 64, diSamples 0 and 2 (the view is drawn with 1), giBounces 2 on a view drawn with 1: the records of the
    override against the rule with that field of its scene changed.  64 samples run on every sixteenth row of the frame: the rule's cost grows with the rays."""
    from sm64rt_legacy_renderer_amd import rt64
    case = GC.make_case(sample_data, name)
    if "di_samples" in over:
        case["view"]["di_samples"] = 1
    s = _open(rt64_lib, case)
    try:
        s.draw(); s.draw()
        img = _images(s, case)
        rows = None
        if over.get("gi_samples", 0) == 64:
            rows = np.zeros((H, W), dtype=bool); rows[::16] = True
        pts, xs, ys = _points(img, rows)
        plain = rt64.sample_indirect(rt64_lib, s.view, pts, _keys(xs, ys, 1))
        records = rt64.sample_indirect(rt64_lib, s.view, pts, _keys(xs, ys, 1), **over)
        spelled = dict(gi_samples=case["view"]["gi_samples"], gi_bounces=case["bounces"], di_samples=case["view"]["di_samples"])
        assert np.array_equal(_bits(rt64.sample_indirect(rt64_lib, s.view, pts, _keys(xs, ys, 1), **spelled)), _bits(plain))          # the frame's own values, spelled out
    finally:
        s.close()
    changed = dict(case)
    changed["view"] = dict(case["view"], **{k: v for k, v in over.items() if k != "gi_bounces"})
    changed["bounces"] = over.get("gi_bounces", case["bounces"])
    if rows is not None:
        img = dict(img); img["id"] = np.where(rows, np.asarray(img["id"]), -1)
    rule = GC.run_rule(changed, 1, img)
    r = _rec(records)
    if over.get("gi_samples") == 0:          # I1: the constant term, no ray
        assert (r["samples"] == 0).all() and not r["moments"].any() and (r["rays"] == 0).all() and (r["flags"] == rt64.INDIRECT_VALID).all()
        ambient = rule["value"][0, 0, :3]
        assert (np.abs(r["indirect"].astype(np.float64) - ambient) <= rule["bound"][0, 0, :3]).all()
        return
    run = dict(records=records, xs=xs, ys=ys)
    raw, mom = _as_images(run, rule["value"], rule["moments"])
    worst, mean, bad = G.compare(raw, mom, rule)
    und = int((~rule["decided"]).sum())
    print("indirect_override %-10s %-22s ratio=%.6f mean=%.6f points=%d undecided=%d" % (name, over, worst, mean, len(r), und))
    assert len(r) == int(rule["surface"].sum()) and int(bad.sum()) == 0 and worst < 1.0, (name, over, worst, int(bad.sum()))
    # gi_cases' cap is a share of the pixels of a frame drawn with the case's sample count, and a pixel is undecided as soon as one of its rays is: with more rays per
    # point the same share of undecided rays leaves that many more points undecided
    more = max(1.0, changed["view"]["gi_samples"] * changed["bounces"] / float(case["view"]["gi_samples"] * case["bounces"]))
    assert und <= int(GC.UNDECIDED_CAP * len(r) * more), (name, over, und)
    if any(spelled[k] != v for k, v in over.items()):
        assert not np.array_equal(_bits(records)[:, :6], _bits(plain)[:, :6])          # (the override matters)
    else:
        assert np.array_equal(_bits(records), _bits(plain))


# ---- 8. forms, sizes, ends ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_forms_sizes_and_the_ends_of_the_arrays(rt64_lib, sample_data):
    """8.  Counts 0, 1, 63, 64, 65, 257 and one above a chunk of the chain equal the prefix of one big call, with the guard words behind `records` and `samples` untouched;
    host arrays against device arrays on the device's stream and on a caller stream, bit-equal; a bad point, a NaN normal, a zero normal and an out-of-range instance in a
    layer record are answered with flags, never with a read."""
    from sm64rt_legacy_renderer_amd import rt64
    case = GC.make_case(sample_data, "two-bounce-layers")
    s = _open(rt64_lib, case)
    hip = ray_rule.Hip()
    try:
        s.draw(); s.draw()
        pts, xs, ys = _points(_images(s, case))
        keys = _keys(xs, ys, 1)
        pts = pts.copy()
        pts[5, 0] = np.inf; pts[6, 5] = np.nan; pts[7, 4:7] = 0.0; pts.view(np.uint32)[8, 3] = rt64.GI_POINT_NONE; pts.view(np.int32)[9, 7] = -1; pts.view(np.int32)[10, 7] = 123456
        host, host_samples = rt64.sample_indirect(rt64_lib, s.view, pts, keys, gi_samples=1, samples=True)
        r, w = _rec(host), _bits(host)
        for i in (5, 6, 7):
            assert r["flags"][i] == rt64.INDIRECT_BAD_POINT and not w[i, [0, 1, 2, 3, 4, 5, 8, 9, 10, 11]].any() and r["instance"][i] == pts.view(np.int32)[i, 7]
            assert not _bits(host_samples)[0, i, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15]].any() and _bits(host_samples)[0, i, 11] == 0xFFFFFFFF          # no ray: instance -1
        assert not w[8, :7].any() and r["instance"][8] == -1 and not w[8, 8:].any()
        assert r["flags"][9] == rt64.INDIRECT_VALID and r["instance"][9] == -1 and r["flags"][10] == rt64.INDIRECT_VALID and r["instance"][10] == 123456          # informational
        assert (r["flags"][11:] == rt64.INDIRECT_VALID).all() and np.isfinite(host[:, :6]).all()
        # host and device forms, records and samples
        d_pts, d_keys = hip.upload(pts), hip.upload(keys)
        sampling = rt64.GI_SAMPLING(1, -1, -1, 0)
        n = len(pts)
        for k, d_k, want in ((keys, d_keys, host), (None, None, rt64.sample_indirect(rt64_lib, s.view, pts, None, gi_samples=1))):
            for st in (None, hip.stream()):
                d_out, d_smp = hip.alloc(want.nbytes), hip.alloc(host_samples.nbytes)
                assert rt64_lib.TraceViewPointsIndirectDevice(s.view, d_pts, d_k, C.addressof(sampling), d_smp, d_out, n, st) == 1, rt64_lib.last_error()
                if st:
                    assert hip.h.hipStreamSynchronize(st) == 0
                assert np.array_equal(_bits(hip.download(d_out, want)), _bits(want))
                if k is not None:
                    assert np.array_equal(_bits(hip.download(d_smp, host_samples)), _bits(host_samples))
        # the links on device arrays
        rays = rt64.gi_rays(rt64_lib, s.view, pts, 1, keys, gi_samples=1)
        assert not rays[5:9].any() and rays[9].any()
        hits, _ = rt64.trace_view_ray_layers(rt64_lib, s.view, rays, 16, flags=CULL)
        hits = hits.copy()
        live = np.nonzero(hits[0].view(np.int32)[:, 3] >= 0)[0]
        a, b, c = live[:3]
        hb = _bits(hits)
        hb[0, a, 3] = 1000; hb[0, b, 4] = 0x7FFFFFFF; hb[0, c, 3] = 0x80000001          # instance past the end, primitive past the end, a negative instance (the list's end)
        shaded = rt64.shade_gi_rays(rt64_lib, s.view, rays, hits, keys)
        sm = _smp(shaded)
        assert sm["flags"][a] == rt64.GI_SAMPLE_VALID | rt64.GI_SAMPLE_BAD_HIT and sm["flags"][b] == rt64.GI_SAMPLE_VALID | rt64.GI_SAMPLE_BAD_HIT and sm["flags"][c] == rt64.GI_SAMPLE_VALID
        assert (sm["instance"][[a, b, c]] == -1).all() and (sm["remaining"][[a, b, c]] == 1.0).all() and np.isfinite(shaded[:, 0:7]).all() and np.isfinite(shaded[:, 8:11]).all()
        assert not _bits(shaded)[5:9][:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15]].any() and (sm["instance"][5:9] == -1).all()
        d_rays, d_hits = hip.upload(rays), hip.upload(hits)
        for st in (None, hip.stream()):
            d_r = hip.alloc(rays.nbytes); d_s = hip.alloc(shaded.nbytes)
            assert rt64_lib.GenerateViewPointGIRaysDevice(s.view, d_pts, d_keys, C.addressof(sampling), 1, 0, d_r, n, st) == 1, rt64_lib.last_error()
            assert rt64_lib.ComposeViewGIRaysDevice(s.view, d_rays, d_hits, 16, d_keys, None, None, d_s, n, st) == 1, rt64_lib.last_error()
            if st:
                assert hip.h.hipStreamSynchronize(st) == 0
            assert np.array_equal(_bits(hip.download(d_r, rays)), _bits(rays)) and np.array_equal(_bits(hip.download(d_s, shaded)), _bits(shaded))
        # sizes: prefixes of one big call, guards behind both outputs.  One sample and one bounce: a chunk of the chain is 2^20 / 16 = 65536 points
        big = (1 << 16) + 1
        reps = -(-(big + 300) // n)
        rng = np.random.default_rng(8)
        order = np.concatenate([np.arange(n)] + [rng.permutation(n) for _ in range(reps - 1)])
        many, many_keys = np.ascontiguousarray(pts[order]), np.ascontiguousarray(keys[order])
        one = rt64.GI_SAMPLING(1, 1, -1, 0)
        whole, whole_samples = rt64.sample_indirect(rt64_lib, s.view, many, many_keys, gi_samples=1, gi_bounces=1, samples=True)
        first = rt64.sample_indirect(rt64_lib, s.view, pts, keys, gi_samples=1, gi_bounces=1)
        assert np.array_equal(_bits(whole), _bits(first)[order])          # a record does not depend on its place, its neighbours or its chunk
        d_many, d_many_keys = hip.upload(many), hip.upload(many_keys)
        guard_r = np.full((len(many), 12), GUARD, dtype=np.uint32); guard_s = np.full((len(many), 16), GUARD, dtype=np.uint32)
        assert rt64_lib.TraceViewPointsIndirectDevice(s.view, d_many, d_many_keys, C.addressof(one), None, hip.upload(guard_r[:4]), 0, None) == 1          # count 0 touches nothing
        for count in (1, 63, 64, 65, 257, big):
            d_r, d_s = hip.upload(guard_r[:count + 258]), hip.upload(guard_s[:count + 258])
            assert rt64_lib.TraceViewPointsIndirectDevice(s.view, d_many, d_many_keys, C.addressof(one), d_s, d_r, count, None) == 1, rt64_lib.last_error()
            out_r, out_s = hip.download(d_r, guard_r[:count + 258]), hip.download(d_s, guard_s[:count + 258])
            assert np.array_equal(out_r[:count], _bits(whole)[:count]) and (out_r[count:] == GUARD).all(), count
            assert np.array_equal(out_s[:count], _bits(whole_samples)[0, :count]) and (out_s[count:] == GUARD).all(), count
            host_r = np.full((count + 258, 12), GUARD, dtype=np.uint32); host_s = np.full((count + 258, 16), GUARD, dtype=np.uint32)
            assert rt64_lib.TraceViewPointsIndirect(s.view, many.ctypes.data, many_keys.ctypes.data, C.addressof(one), host_s.ctypes.data, host_r.ctypes.data, count) == 1, rt64_lib.last_error()
            assert np.array_equal(host_r, out_r) and np.array_equal(host_s, out_s), count
    finally:
        hip.close()
        s.close()


# ---- 9. refusals and counters ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(rt64_lib, sample_data):
    """9a.  Every out-of-range sampling field, flags != 0, a view without a drawn frame, count > width * height with keys = NULL and misaligned device pointers are refused with
    the function's name in RT64_GetLastError; count = 0 succeeds and touches nothing."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    case = GC.make_case(sample_data, "opaque-3")
    R_ = rt64_lib
    s = sample_scene.Rt64Scene(rt64_lib, case["data_at"](0), W, H, hip_device=0)
    hip = ray_rule.Hip()
    try:
        s.set_view_description(denoiser=False, **case["view"])
        n = 64
        pts = np.zeros((n, 8), dtype=np.float32); pts[:, 5] = 1.0
        keys = _keys(np.arange(n), np.zeros(n), 0)
        rays = np.zeros((n, 8), dtype=np.float32); hits = np.zeros((16 * n, 8), dtype=np.float32)
        out = np.full((n, 16), GUARD, dtype=np.uint32)
        d_pts, d_keys, d_rays, d_hits, d_out = hip.upload(pts), hip.upload(keys), hip.upload(rays), hip.upload(hits), hip.upload(out)
        p_, k_, r_, h_, o_ = pts.ctypes.data, keys.ctypes.data, rays.ctypes.data, hits.ctypes.data, out.ctypes.data
        names = {"g": "RT64_GenerateViewPointGIRays", "gd": "RT64_GenerateViewPointGIRaysDevice", "c": "RT64_ComposeViewGIRays", "cd": "RT64_ComposeViewGIRaysDevice",
                 "t": "RT64_TraceViewPointsIndirect", "td": "RT64_TraceViewPointsIndirectDevice", "r": "RT64_TraceViewRayIndirect"}

        def calls(sampling=None, count=n, keys_host=k_, keys_dev=d_keys):
            return {"g": lambda: R_.GenerateViewPointGIRays(s.view, p_, keys_host, sampling, 1, 0, o_, count),
                    "gd": lambda: R_.GenerateViewPointGIRaysDevice(s.view, d_pts, keys_dev, sampling, 1, 0, d_out, count, None),
                    "c": lambda: R_.ComposeViewGIRays(s.view, r_, h_, 16, keys_host, None, sampling, o_, count),
                    "cd": lambda: R_.ComposeViewGIRaysDevice(s.view, d_rays, d_hits, 16, keys_dev, None, sampling, d_out, count, None),
                    "t": lambda: R_.TraceViewPointsIndirect(s.view, p_, keys_host, sampling, None, o_, count),
                    "td": lambda: R_.TraceViewPointsIndirectDevice(s.view, d_pts, keys_dev, sampling, None, d_out, count, None),
                    "r": lambda: R_.TraceViewRayIndirect(s.view, r_, None, None, keys_host, sampling, o_, count, 0)}

        def refused(word, which, call):
            ok = call()
            assert ok == 0 and R_.last_error().startswith(names[which] + ":") and word in R_.last_error(), (which, ok, R_.last_error())

        def all_refused(word, **kw):
            for which, call in calls(**kw).items():
                refused(word, which, call)
        all_refused("draw")                                                               # before the first frame
        s.draw()
        for which, call in calls(count=0).items():
            assert call() == 1, (which, R_.last_error())
        for bad, word in (((65, -1, -1, 0), "giSamples"), ((-2, -1, -1, 0), "giSamples"), ((-1, 0, -1, 0), "giBounces"), ((-1, 3, -1, 0), "giBounces"), ((-1, -2, -1, 0), "giBounces"),
                          ((-1, -1, 65, 0), "diSamples"), ((-1, -1, -2, 0), "diSamples"), ((-1, -1, -1, 1), "sampling flags")):
            p = rt64.GI_SAMPLING(*bad)
            all_refused(word, sampling=C.addressof(p))
        edge = rt64.GI_SAMPLING(64, 2, 64, 0)                                             # the largest accepted values
        assert R_.TraceViewPointsIndirectDevice(s.view, d_pts, d_keys, C.addressof(edge), None, d_out, 4, None) == 1, R_.last_error()
        none = rt64.GI_SAMPLING(0, -1, -1, 0)
        refused("giSamples", "g", lambda: R_.GenerateViewPointGIRays(s.view, p_, k_, C.addressof(none), 1, 0, o_, n))
        refused("slot", "g", lambda: R_.GenerateViewPointGIRays(s.view, p_, k_, None, 0, 0, o_, n))
        refused("slot", "gd", lambda: R_.GenerateViewPointGIRaysDevice(s.view, d_pts, d_keys, None, 4, 0, d_out, n, None))          # the view has 3 samples
        refused("unknown flags", "g", lambda: R_.GenerateViewPointGIRays(s.view, p_, k_, None, 1, 2, o_, n))
        refused("unknown flags", "r", lambda: R_.TraceViewRayIndirect(s.view, r_, None, None, k_, None, o_, n, ray_rule.ACCEPT_FIRST_HIT))
        refused("maxLayers", "c", lambda: R_.ComposeViewGIRays(s.view, r_, h_, 0, k_, None, None, o_, n))
        refused("maxLayers", "cd", lambda: R_.ComposeViewGIRaysDevice(s.view, d_rays, d_hits, 17, d_keys, None, None, d_out, n, None))
        refused("NULL view", "t", lambda: R_.TraceViewPointsIndirect(None, p_, k_, None, None, o_, n))
        refused("NULL", "t", lambda: R_.TraceViewPointsIndirect(s.view, None, k_, None, None, o_, n))
        refused("NULL", "t", lambda: R_.TraceViewPointsIndirect(s.view, p_, k_, None, None, None, n))
        refused("NULL", "g", lambda: R_.GenerateViewPointGIRays(s.view, p_, k_, None, 1, 0, None, n))
        refused("NULL", "c", lambda: R_.ComposeViewGIRays(s.view, r_, None, 16, k_, None, None, o_, n))
        refused("NULL", "r", lambda: R_.TraceViewRayIndirect(s.view, None, None, None, k_, None, o_, n, 0))
        # keys = NULL counts the frame's pixels
        pixels = W * H
        frame_pts = np.zeros((pixels + 1, 8), dtype=np.float32); frame_pts.view(np.uint32)[:, 3] = rt64.GI_POINT_NONE
        frame_out = np.zeros((pixels + 1, 16), dtype=np.float32)
        assert R_.TraceViewPointsIndirect(s.view, frame_pts.ctypes.data, None, None, None, frame_out.ctypes.data, pixels) == 1, R_.last_error()
        refused("pixels", "t", lambda: R_.TraceViewPointsIndirect(s.view, frame_pts.ctypes.data, None, None, None, frame_out.ctypes.data, pixels + 1))
        refused("pixels", "g", lambda: R_.GenerateViewPointGIRays(s.view, frame_pts.ctypes.data, None, None, 1, 0, frame_out.ctypes.data, pixels + 1))
        refused("pixels", "r", lambda: R_.TraceViewRayIndirect(s.view, frame_pts.ctypes.data, None, None, None, None, frame_out.ctypes.data, pixels + 1, 0))
        # misaligned device pointers
        refused("aligned", "td", lambda: R_.TraceViewPointsIndirectDevice(s.view, d_pts + 4, d_keys, None, None, d_out, 4, None))
        refused("aligned", "td", lambda: R_.TraceViewPointsIndirectDevice(s.view, d_pts, d_keys + 8, None, None, d_out, 4, None))
        refused("aligned", "td", lambda: R_.TraceViewPointsIndirectDevice(s.view, d_pts, d_keys, None, d_out + 4, d_out, 4, None))
        refused("aligned", "td", lambda: R_.TraceViewPointsIndirectDevice(s.view, d_pts, d_keys, None, None, d_out + 4, 4, None))
        refused("aligned", "gd", lambda: R_.GenerateViewPointGIRaysDevice(s.view, d_pts, d_keys, None, 1, 0, d_out + 8, 4, None))
        refused("aligned", "cd", lambda: R_.ComposeViewGIRaysDevice(s.view, d_rays, d_hits + 4, 16, d_keys, None, None, d_out, 4, None))
        refused("aligned", "cd", lambda: R_.ComposeViewGIRaysDevice(s.view, d_rays, d_hits, 16, d_keys, d_out + 2, None, d_out, 4, None))
        assert (out == GUARD).all()
        m = case["data_at"](0).meshes[case["data_at"](0).instances[1].mesh]
        s.set_mesh(s.meshes[case["data_at"](0).instances[1].mesh], m.vertices, m.indices)
        for which in ("c", "cd", "t", "td", "r"):
            refused("RT64_SetMesh", which, calls()[which])
    finally:
        hip.close()
        s.close()


def test_counters_follow_count_traversal(rt64_lib, sample_data):
    """9b.  nodesVisited and trianglesTested are 0 without count_traversal and positive with it on the points whose rays were walked; the other fields do not change."""
    from sm64rt_legacy_renderer_amd import rt64
    case = GC.make_case(sample_data, "two-bounce-layers")
    s = _open(rt64_lib, case)
    try:
        s.draw(); s.draw()
        pts, xs, ys = _points(_images(s, case))
        keys = _keys(xs, ys, 1)
        a, a_s = rt64.sample_indirect(rt64_lib, s.view, pts, keys, gi_samples=1, samples=True)
        assert s.option("count_traversal", 1)
        s.draw()
        b, b_s = rt64.sample_indirect(rt64_lib, s.view, pts, keys, gi_samples=1, samples=True)
    finally:
        s.close()
    ra, rb = _rec(a), _rec(b)
    assert not ra["nodesVisited"].any() and not ra["trianglesTested"].any() and not _bits(a_s)[..., 14:16].any()
    assert np.array_equal(_bits(a)[:, :9], _bits(b)[:, :9]) and np.array_equal(_bits(a_s)[..., :14], _bits(b_s)[..., :14])
    assert (rb["nodesVisited"] > 0).all() and (rb["trianglesTested"] > 0).sum() > 1000
    lit = (_smp(b_s)["flags"][0] & (rt64.GI_SAMPLE_SURFACE | rt64.GI_SAMPLE_UNLIT)) == rt64.GI_SAMPLE_SURFACE
    assert lit.sum() > 500 and (_smp(b_s)["nodesVisited"][0][lit] > 0).all() and not _smp(b_s)["nodesVisited"][0][~(( _smp(b_s)["flags"][0] & rt64.GI_SAMPLE_SURFACE) != 0)].any()
