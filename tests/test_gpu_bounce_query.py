"""The frame's mirror and glass rays for ray-query hits and mirror chains (include/rt64_bounce.h) on the GPU, held to the float64 rule of tests/bounce_rule.py
record by record (rules R1-R12), to the one-step calls a chain replaces (R7), to the frame's own primary resolve (R9), and to themselves: the forms
agree byte for byte, a NULL output changes no other, nothing is written past the last record, bad calls are refused as R10 says.

One run's lines of the first and the R9 test are committed as profiles/bounce_rule_deviation.txt.
"""
import numpy as np
import pytest

import bounce_cases as BC
import bounce_rule as R
import light_cases as LC
import light_rule as L
import lighting_cases
import material_cases as MC
import material_rule as M
import mirror_cases as MRC
import mirror_rule as MR
import ray_rule

pytestmark = pytest.mark.gpu

CULL, FIRST = ray_rule.CULL_BACK_FACING, ray_rule.ACCEPT_FIRST_HIT
W, H = lighting_cases.W, lighting_cases.H
MISS_HIT = np.array([0x7F800000, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0], dtype=np.uint32)          # Q5: t = +inf, instance -1
MISS_RECORD = np.array([0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0], dtype=np.uint32)                # R1


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


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BC.NAMES)
def test_the_records_lie_within_the_rule(rt64_lib, oracle_lib, sample_data, name):
    """1.  Every case: RT64_BounceViewRayHits on the hits of RT64_TraceViewRaysAlpha: fresnel, position and both directions within the bound on every decided record;
    flags, instance, primitive, the factors, tMin and tMax exact; undecided records at most 2 % of the real hits; the one-call form equal to walk + records byte for
    byte; an output switched off leaves the others the same bytes; each mutation assigned to the case leaves its bound against the device's records."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, flags = BC.make_case(sample_data, name)
    rays, lods = BC.rays_and_lods(data, name, seed, options)
    s = _open(rt64_lib, data, options)
    try:
        s.draw()
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods, flags)
        got = rt64.bounce_view_ray_hits(rt64_lib, s.view, rays, hits, lods)
        one = rt64.trace_view_ray_bounces(rt64_lib, s.view, rays, lods, flags)
        assert _same(one, (hits,) + got), name
        assert np.array_equal(_bits(rt64.trace_view_ray_bounces(rt64_lib, s.view, rays, lods, flags, bounces=False, refracted=False)[1]), _bits(got[1]))
        assert np.array_equal(_bits(rt64.bounce_view_ray_hits(rt64_lib, s.view, rays, hits, lods, reflected=False, refracted=False)), _bits(got[0]))
        assert _same(rt64.bounce_view_ray_hits(rt64_lib, s.view, rays, hits, lods, reflected=False), (got[0], got[2]))
        assert _same(rt64.bounce_view_ray_hits(rt64_lib, s.view, rays, hits, lods, bounces=False), (got[1], got[2]))
    finally:
        s.close()
    levels = M.texture_levels(data, MC.mipmapped(options))
    rule = R.bounces(data, levels, rays, hits, lods)
    ratios, exact = R.compare(rule, got)
    print(R.report(name, rule, ratios, exact))
    assert exact.all(), (name, np.nonzero(~exact)[0][:8].tolist())
    for k, r in ratios.items():
        assert (r <= 1.0).all(), (name, k, float(r.max()), np.nonzero(~(r <= 1.0))[0][:8].tolist())
    sh = R.shares(rule)
    assert (rule["kind"] == 2).sum() >= 400
    assert all(a >= b for a, b in zip(sh[:5], BC.SHARES[name])), (sh, BC.SHARES[name])
    assert sh[5] <= BC.UNDECIDED_CAP, sh
    for mutation, where in BC.MUTATION_CASE.items():
        if where != name:
            continue
        wrong = R.bounces(data, levels, rays, hits, lods, mutate=mutation)
        with np.errstate(invalid="ignore"):
            ratios, exact = R.compare(wrong, got)
        out = ~exact
        for r in ratios.values():
            out |= ~(r <= 1.0)
        und = int((wrong["undecided"] | rule["undecided"]).sum())
        print("    mutation %-24s %4d of %4d of the device's records outside its bound (undecided with either rule: %d)" % (mutation, int(out.sum()), len(out), und))
        assert out.sum() > und, mutation


# ---- 2. forms, sizes, R1 ---------------------------------------------------------------------------------------------------------------------------------------------

def test_forms_sizes_and_the_end_of_the_arrays(rt64_lib, sample_data):
    """2.  Host arrays, device arrays on the device's stream and on a caller stream: the same bytes; counts 1, 63, 65, 257 and RT_GRID_BLOCKS x RT_BLOCK + 1 (the
    grid-stride loop) equal the prefix of one big call with the guard words behind the last record untouched; misses, bad hits and NaN rays give R1's records, and
    the all-zero rays of a miss trace as misses."""
    from sm64rt_legacy_renderer_amd import rt64
    name = "mapped mirrors"
    data, seed, options, flags = BC.make_case(sample_data, name)
    rays, lods = BC.rays_and_lods(data, name, seed, options)
    s = _open(rt64_lib, data, options)
    hip = ray_rule.Hip()
    try:
        s.draw()
        rays[7, 0] = np.nan; rays[8, 5] = np.nan; rays[9, 7] = np.nan
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods)
        hb = _bits(hits)
        assert (hb[7:10, 3] == 0xFFFFFFFF).all()                                               # Q6: a NaN ray misses
        hb[3, 3] = 1000; hb[4, 3] = 0; hb[4, 4] = 0x7FFFFFFF; hb[5, 3] = 0x80000001           # R1: instance past the end, primitive past the end, a negative instance
        host = rt64.bounce_view_ray_hits(rt64_lib, s.view, rays, hits, lods)
        b = _bits(host[0])
        miss = b[:, 4] == 0xFFFFFFFF
        assert (b[miss][:, [0, 1, 2, 6, 7]] == 0).all() and (b[miss, 5] == 0xFFFFFFFF).all() and set(b[miss, 3].tolist()) <= {0, R.BAD_HIT}
        assert b[3, 3] == R.BAD_HIT and b[4, 3] == R.BAD_HIT and b[5, 3] == 0 and miss[[3, 4, 5, 7, 8, 9]].all()
        assert not _bits(host[1])[miss].any() and not _bits(host[2])[miss].any() and 100 < miss.sum() < len(rays) - 400
        again = _bits(rt64.trace_rays_alpha(rt64_lib, s.view, np.ascontiguousarray(host[1][miss])))
        assert (again[:, 3] == 0xFFFFFFFF).all() and (again[:, 0] == 0x7F800000).all()          # Q6: no direction, tMin = tMax: a miss without a walk
        assert _same(rt64.bounce_view_ray_hits(rt64_lib, s.view, rays, hits, np.zeros(len(rays), dtype=np.float32)), rt64.bounce_view_ray_hits(rt64_lib, s.view, rays, hits))
        d_rays, d_hits, d_lods = hip.upload(rays), hip.upload(hits), hip.upload(lods)
        for st in (None, hip.stream()):
            d_out = [hip.alloc(a.nbytes) for a in host]
            assert rt64_lib.BounceViewRayHitsDevice(s.view, d_rays, d_hits, d_lods, d_out[0], d_out[1], d_out[2], len(rays), st) == 1, rt64_lib.last_error()
            if st:
                assert hip.h.hipStreamSynchronize(st) == 0
            assert _same([hip.download(d, a) for d, a in zip(d_out, host)], host)
        big = 2048 * 256 + 1
        reps = -(-(big + 300) // len(rays))
        rng = np.random.default_rng(6)
        order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(reps - 1)])          # later repetitions shuffled: waves mix instances
        many, many_hits, many_lods = np.ascontiguousarray(rays[order]), np.ascontiguousarray(hits[order]), np.ascontiguousarray(lods[order])
        whole = rt64.bounce_view_ray_hits(rt64_lib, s.view, many, many_hits, many_lods)          # host form: chunks of 2^18
        assert _same(whole, [a[order] for a in host])                                              # a record does not depend on its place or its neighbours
        d_rays, d_hits, d_lods = hip.upload(many), hip.upload(many_hits), hip.upload(many_lods)
        guard = np.full((len(many), 8), 0xABABABAB, dtype=np.uint32)
        for count in (1, 63, 65, 257, big):
            d_guard = [hip.upload(guard[:count + 258]) for _ in range(3)]
            assert rt64_lib.BounceViewRayHitsDevice(s.view, d_rays, d_hits, d_lods, d_guard[0], d_guard[1], d_guard[2], count, None) == 1, rt64_lib.last_error()
            for d, w_ in zip(d_guard, whole):
                out = hip.download(d, guard[:count + 258])
                assert np.array_equal(out[:count], _bits(w_)[:count]) and (out[count:] == 0xABABABAB).all(), count
    finally:
        hip.close()
        s.close()


def _repeated(rays, lods, count, seed):
    """`count` rays made of the case's rays over and over, the later repetitions shuffled."""
    rng = np.random.default_rng(seed)
    order = np.concatenate([np.arange(len(rays))] + [rng.permutation(len(rays)) for _ in range(-(-count // len(rays)) - 1)])[:count]
    return np.ascontiguousarray(rays[order]), np.ascontiguousarray(lods[order])


def _guarded(records, spare=7):
    return np.full((records + spare, 8), 0xABABABAB, dtype=np.uint32)


def test_host_chains_that_cross_a_chunk_agree_with_the_device_form(rt64_lib, sample_data):
    """2b.  A host chain of depth 8 stages 2^18 / 8 = 32768 rays per round trip and scatters each chunk's eight blocks to the caller's segment-major arrays: 65 rays
    more than a chunk, with lods, equal the device form -- which does not chunk -- bit for bit, and the spare records behind both arrays keep their guard words."""
    name, depth, count = "mapped mirrors", 8, 32768 + 65
    data, seed, options, flags = BC.make_case(sample_data, name)
    rays, lods = BC.rays_and_lods(data, name, seed, options)
    many, many_lods = _repeated(rays, lods, count, 16)
    s = _open(rt64_lib, data, options)
    hip = ray_rule.Hip()
    try:
        s.draw()
        d_rays, d_lods, d_hits, d_rec = hip.upload(many), hip.upload(many_lods), hip.alloc(depth * count * 32), hip.alloc(depth * count * 32)
        assert rt64_lib.TraceViewRayMirrorChainsDevice(s.view, d_rays, d_lods, depth, d_hits, d_rec, count, flags & CULL, None) == 1, rt64_lib.last_error()
        want = [hip.download(d, np.empty((depth * count, 8), dtype=np.uint32)) for d in (d_hits, d_rec)]
        assert ((want[1].reshape(depth, count, 8)[1, :, 3] & R.VALID) != 0).sum() >= 32          # chains that go on behind segment 0
        host = [_guarded(depth * count), _guarded(depth * count)]
        assert rt64_lib.TraceViewRayMirrorChains(s.view, many.ctypes.data, many_lods.ctypes.data, depth, host[0].ctypes.data, host[1].ctypes.data, count, flags & CULL) == 1, rt64_lib.last_error()
        for out, w in zip(host, want):
            assert np.array_equal(out[:len(w)], w) and (out[len(w):] == 0xABABABAB).all()
    finally:
        hip.close()
        s.close()


def test_a_host_walk_with_records_that_crosses_a_chunk_is_the_two_device_calls(rt64_lib, sample_data):
    """2c.  RT64_TraceViewRayBounces (host arrays only) at 2^18 + 65 rays, one chunk and 65: with all four outputs, and with `reflected` alone (hits = NULL: the walk's
    hits never leave the device), it equals RT64_TraceViewRaysAlphaDevice followed by RT64_BounceViewRayHitsDevice bit for bit; the spare records behind every
    array keep their guard words."""
    name, count = "mapped mirrors", (1 << 18) + 65
    data, seed, options, flags = BC.make_case(sample_data, name)
    rays, lods = BC.rays_and_lods(data, name, seed, options)
    many, many_lods = _repeated(rays, lods, count, 17)
    s = _open(rt64_lib, data, options)
    hip = ray_rule.Hip()
    try:
        s.draw()
        d_rays, d_lods = hip.upload(many), hip.upload(many_lods)
        d_out = [hip.alloc(count * 32) for _ in range(4)]          # hits, bounces, reflected, refracted
        assert rt64_lib.TraceViewRaysAlphaDevice(s.view, d_rays, d_lods, d_out[0], count, flags, None) == 1, rt64_lib.last_error()
        assert rt64_lib.BounceViewRayHitsDevice(s.view, d_rays, d_out[0], d_lods, d_out[1], d_out[2], d_out[3], count, None) == 1, rt64_lib.last_error()
        want = [hip.download(d, np.empty((count, 8), dtype=np.uint32)) for d in d_out]
        assert (want[1][:, 4] != 0xFFFFFFFF).sum() > count // 100 and want[2].any()          # real hits with rays reflected off them
        host = [_guarded(count) for _ in range(4)]
        rp, lp = many.ctypes.data, many_lods.ctypes.data
        assert rt64_lib.TraceViewRayBounces(s.view, rp, host[0].ctypes.data, lp, host[1].ctypes.data, host[2].ctypes.data, host[3].ctypes.data, count, flags) == 1, rt64_lib.last_error()
        for out, w in zip(host, want):
            assert np.array_equal(out[:count], w) and (out[count:] == 0xABABABAB).all()
        alone = _guarded(count)
        assert rt64_lib.TraceViewRayBounces(s.view, rp, None, lp, None, alone.ctypes.data, None, count, flags) == 1, rt64_lib.last_error()
        assert np.array_equal(alone[:count], want[2]) and (alone[count:] == 0xABABABAB).all()
    finally:
        hip.close()
        s.close()


def test_uniform_and_mixed_waves_give_the_same_records(rt64_lib, sample_data):
    """3.  lighting_cases' 66 instances: the hits sorted by instance (waves of 64 hits that share one: the scalar read of the instance) and the same hits shuffled
    (mixed waves: the per-lane gather), and a batch that starts with waves made of one hit of each of 64 different instances, give the same record for the same hit."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, heights = lighting_cases.make_case(sample_data, "66 instances, 20 lights")
    for i in data.instances:
        i.material.reflectionFactor = 0.25; i.material.refractionFactor = 0.75
    rng = np.random.default_rng(12)
    rays = np.concatenate([lighting_cases.rays_and_lods(data, seed, options, heights)[0], BC.aimed_rays(data, rng, 6000)]).astype(np.float32)
    s = _open(rt64_lib, data, options)
    try:
        s.draw()
        hits = rt64.trace_rays_alpha(rt64_lib, s.view, rays)
        inst = hits.view(np.int32)[:, 3]
        by_instance = np.argsort(inst, kind="stable")
        a = rt64.bounce_view_ray_hits(rt64_lib, s.view, np.ascontiguousarray(rays[by_instance]), np.ascontiguousarray(hits[by_instance]))
        shuffled = rng.permutation(len(rays))
        b = rt64.bounce_view_ray_hits(rt64_lib, s.view, np.ascontiguousarray(rays[shuffled]), np.ascontiguousarray(hits[shuffled]))
        # waves of 64 DIFFERENT instances: records 64 w .. 64 w + 63 are one hit of each of the 64 instances with the most hits, as many waves as the 64th has
        # hits; the rest of the batch behind them as it is
        ids, counts = np.unique(inst[inst >= 0], return_counts=True)
        assert len(ids) >= 64
        top = ids[np.argsort(-counts, kind="stable")[:64]]
        full = int(counts[np.argsort(-counts, kind="stable")[63]])
        columns = np.stack([np.nonzero(inst == k)[0][:full] for k in top], axis=1)          # (full, 64): row w is wave w
        each = np.concatenate([columns.reshape(-1), np.setdiff1d(np.arange(len(rays)), columns.reshape(-1))])
        c = rt64.bounce_view_ray_hits(rt64_lib, s.view, np.ascontiguousarray(rays[each]), np.ascontiguousarray(hits[each]))
    finally:
        s.close()
    back_a, back_b, back_c = np.argsort(by_instance), np.argsort(shuffled), np.argsort(each)
    assert _same([x[back_a] for x in a], [x[back_b] for x in b])
    assert len(each) == len(rays) and full >= 1 and all(len(set(w.tolist())) == 64 for w in inst[each][: 64 * full].reshape(full, 64))
    assert _same([x[back_c] for x in c], [x[back_a] for x in a])
    assert all((_bits(x)[: 64 * full] != 0).any() for x in c)
    sorted_inst = inst[by_instance]
    waves = sorted_inst[: len(sorted_inst) // 64 * 64].reshape(-1, 64)
    uniform = ((waves == waves[:, :1]).all(axis=1) & (waves[:, 0] >= 0)).sum()
    mixed = max(len(set(w.tolist())) for w in inst[shuffled][: len(inst) // 64 * 64].reshape(-1, 64))
    print("66 instances: %d hits on %d instances; sorted: %d waves on one instance; shuffled: up to %d instances in a wave; %d waves of 64 different instances" %
          ((inst >= 0).sum(), len(set(inst[inst >= 0].tolist())), uniform, mixed, full))
    assert uniform >= 10 and mixed >= 12 and len(set(inst[inst >= 0].tolist())) >= 40


# ---- 4. chains (R7) ----------------------------------------------------------------------------------------------------------------------------------------------------

REACH = {"facing": 0.05, "floor": 0.0, "fence over a mirror": 0.0}          # rays that reach segment 7: the facing mirrors keep a twentieth of the batch at the least


@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("name", sorted(REACH))
def test_chains_are_the_iterated_one_step_calls(rt64_lib, sample_data, name, cache):
    """4.  R7 at depth 1, 2 and 8, with the LDS scene cache and without it: segment 0 is RT64_TraceViewRaysAlpha; segment s + 1 is RT64_TraceViewRayBounces on
    segment s's reflected rays wherever segment s is MIRROR, byte for byte; every later segment of an ended chain holds the miss hit and the miss record;
    CONTINUED is set exactly where the successor was walked; the device form equals the host form."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, flags = BC.make_case(sample_data, name)
    rays, lods = BC.rays_and_lods(data, name, seed, options)
    if name == "facing":          # rays between the floor and the ceiling that faces it, going up and down: the chains that last
        rng = np.random.default_rng(9)
        n = 600
        o = np.stack([rng.uniform(4.0, 8.0, n), rng.uniform(0.1, 0.4, n), rng.uniform(-2.0, 4.0, n)], axis=1)
        d = np.stack([rng.uniform(-0.05, 0.05, n), rng.choice([-1.0, 1.0], n), rng.uniform(-0.05, 0.05, n)], axis=1) * rng.uniform(0.5, 2.0, (n, 1))
        rays = np.ascontiguousarray(np.concatenate([rays, BC._pack(o, d)]).astype(np.float32))
    n = len(rays)
    s = _open(rt64_lib, data, dict(options, lds_cache=cache))
    hip = ray_rule.Hip()
    try:
        s.draw()
        first = rt64.trace_rays_alpha(rt64_lib, s.view, rays, lods, flags)
        # the iterated one-step calls, eight deep
        want_hits, want_rec = [], []
        cur, cur_lods, alive = rays, lods, np.ones(n, dtype=bool)
        for seg in range(8):
            h, rec, refl, _ = rt64.trace_view_ray_bounces(rt64_lib, s.view, cur, cur_lods, flags)
            hb, rb = _bits(h).copy(), _bits(rec).copy()
            hb[~alive] = MISS_HIT; rb[~alive] = MISS_RECORD
            want_hits.append(hb); want_rec.append(rb)
            alive = alive & ((rb[:, 3] & R.MIRROR) != 0)
            cur, cur_lods = refl, None
        assert np.array_equal(want_hits[0], _bits(first))
        lengths = None
        for depth in (1, 2, 8):
            hits, rec = rt64.trace_view_ray_mirror_chains(rt64_lib, s.view, rays, depth, lods, flags)
            assert hits.shape == (depth, n, 8) and rec.shape == (depth, n, 8)
            hb, rb = _bits(hits), _bits(rec)
            for seg in range(depth):
                goes_on = ((want_rec[seg][:, 3] & R.MIRROR) != 0) & (seg + 1 < depth)
                want = want_rec[seg].copy(); want[goes_on, 3] |= R.CONTINUED
                assert np.array_equal(hb[seg], want_hits[seg]), (depth, seg, np.nonzero((hb[seg] != want_hits[seg]).any(axis=1))[0][:8].tolist())
                assert np.array_equal(rb[seg], want), (depth, seg, np.nonzero((rb[seg] != want).any(axis=1))[0][:8].tolist())
            d_hits, d_rec = hip.alloc(hits.nbytes), hip.alloc(rec.nbytes)
            d_rays, d_lods = hip.upload(rays), (hip.upload(lods) if lods is not None else None)
            assert rt64_lib.TraceViewRayMirrorChainsDevice(s.view, d_rays, d_lods, depth, d_hits, d_rec, n, flags, None) == 1, rt64_lib.last_error()
            assert np.array_equal(_bits(hip.download(d_hits, hits)), hb) and np.array_equal(_bits(hip.download(d_rec, rec)), rb)
            if depth == 8:
                lengths = ((rb[:, :, 3] & R.VALID) != 0).sum(axis=0)
        reached = float((lengths == 8).mean())
        per_wave = lengths[: n // 64 * 64].reshape(-1, 64)
        spread = int(sum(len(set(w.tolist())) >= 3 for w in per_wave))
        print("chains %-20s lds_cache=%d rays %d  lengths %s  reach segment 7: %.3f  waves with three or more different lengths: %d of %d" %
              (name, cache, n, np.bincount(lengths, minlength=9).tolist(), reached, spread, len(per_wave)))
        assert reached >= REACH[name]
        if name == "floor":
            assert spread >= len(per_wave) // 2          # chains end at different depths inside one wave
    finally:
        hip.close()
        s.close()


# ---- 5. the frame (R9) ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["floor", "glass", "depth bias"])
def test_camera_rays_agree_with_the_frame(rt64_lib, sample_data, name):
    """5.  A frame without reflection passes at 88 x 72, the camera rays of RT64_GenerateViewCameraRays for every pixel: on the pixels whose first K2 hit lies on the
    instance the frame kept (at least 98 % of the shaded ones) position is RT64_IMAGE_SHADING_POSITION within the float32 bound of R2 (bit equality is reported),
    reflected and refracted lie within what half a step of the stored view direction (f16) and normal (SNORM16 in the frame's hit record, then f16) gives through
    reflect / refract plus the record's own bound,
    and on those whose surface is opaque and unfogged fresnel is the RT64_IMAGE_REFLECTION alpha within the rule's error plus half an f16 step."""
    from sm64rt_legacy_renderer_amd import rt64
    if name == "depth bias":          # bounce_cases' own: the mirror floor (opaque, unfogged) with depthBias 0.25, the sphere with -0.125
        case = dict(view=dict(di_samples=0, max_lights=12))
        data = BC.make_case(sample_data, name)[0]
    else:
        case = MRC.make_case(MC.small_sample(sample_data), name)
        data = case["data_at"](0)
    w, h = LC.W, LC.H
    s = _open(rt64_lib, data, {"lean_frames": 0}, w, h)
    try:
        s.set_view_description(**case["view"])
        assert s.option("max_reflections", 0)
        s.draw()
        img = {k: s.readback(getattr(rt64, "IMAGE_" + k)) for k in ("SHADING_POSITION", "VIEW_DIRECTION", "SHADING_NORMAL", "INSTANCE_ID", "REFLECTION")}
        pixels = np.stack(np.meshgrid(np.arange(w), np.arange(h), indexing="xy"), axis=-1).reshape(-1, 2).astype(np.uint32)
        rays = rt64.camera_rays(rt64_lib, s.view, pixels, differentials=False)
        hits, rec, refl, refr = rt64.trace_view_ray_bounces(rt64_lib, s.view, rays, None, CULL)
    finally:
        s.close()
    rule = R.bounces(data, M.texture_levels(data), rays, hits)
    inst = img["INSTANCE_ID"].reshape(h, w).astype(np.int64)
    tab = R.material_table(data)
    g = R.at_gbuffer(img["SHADING_POSITION"], img["VIEW_DIRECTION"], img["SHADING_NORMAL"], inst, tab, half_step=L.F16_HALF_STEP, normal_step=MR.SNORM16_HALF_STEP)
    lit = g["lit"].reshape(-1)
    mine = rec.view(np.int32)[:, 4]
    decided = (rule["kind"] == 2) & ~rule["undecided"]
    sp = img["SHADING_POSITION"].reshape(-1, 4)[:, :3]
    pv, pe = rule["position"]
    kept = lit & decided & (mine == inst.reshape(-1))          # the first K2 hit is on the instance the frame kept
    bit_equal = (_bits(sp) == _bits(refl[:, 0:3])).all(axis=1)
    ratio_p = (np.abs(sp.astype(np.float64) - pv) / pe).max(axis=1)
    at = np.cumsum(lit) - 1                                                   # row of a lit pixel in g's arrays
    f16_only = R.at_gbuffer(img["SHADING_POSITION"], img["VIEW_DIRECTION"], img["SHADING_NORMAL"], inst, tab, half_step=L.F16_HALF_STEP)
    ratios, without = {}, {}
    for key, got in (("reflected", refl[:, 4:7]), ("refracted", refr[:, 4:7])):
        v, e = g[key]
        dev = np.abs(got[kept].astype(np.float64) - v[at[kept]])
        ratios[key] = (dev / (e[at[kept]] + rule[key][1][kept])).max(axis=1)
        without[key] = (dev / (f16_only[key][1][at[kept]] + rule[key][1][kept])).max(axis=1)          # reported, not asserted: the bound without the SNORM16 step
    tir_same = (g["total"][at[kept]] == ((_bits(rec)[kept, 3] & R.TOTAL_INTERNAL) != 0)) | g["tir_undecided"][at[kept]]
    solid = np.asarray([float(data.instances[i].material.solidAlphaMultiplier) >= 1.0 and not data.instances[i].material.fogEnabled
                        for i in __import__("surface_rule").raytraced_instances(data)])
    plain = kept & solid[np.where(mine >= 0, mine, 0)]
    alpha = img["REFLECTION"].reshape(-1, 4)[:, 3].astype(np.float64)
    fv, fe = rule["fresnel"]
    fb = fe[:, 0] + np.maximum(L.F16_HALF_STEP * (np.abs(fv[:, 0]) + fe[:, 0]), L.F16_FLOOR)
    ratio_f = np.abs(alpha - rec[:, 0].astype(np.float64)) / fb
    print("frame %-6s shaded %4d kept %4d opaque and unfogged %4d  position bit-equal on %d of %d, ratio max %.3f  fresnel ratio max %.3f  reflected %.3f  refracted %.3f  (with f16 half steps alone: %.3f, %.3f)  biased pixels %d  total internal %d" %
          (name, int(lit.sum()), int(kept.sum()), int(plain.sum()), int(bit_equal[kept].sum()), int(kept.sum()), ratio_p[kept].max(), ratio_f[plain].max(initial=0.0),
           ratios["reflected"].max(), ratios["refracted"].max(), without["reflected"].max(), without["refracted"].max(),
           int((tab["depthBias"][np.where(mine >= 0, mine, 0)][kept] != 0.0).sum()), int(((_bits(rec)[kept, 3] & R.TOTAL_INTERNAL) != 0).sum())))
    assert kept.sum() >= 2900 and kept.sum() >= 0.98 * lit.sum() and (ratio_p[kept] <= 1.0).all()
    assert (ratios["reflected"] <= 1.0).all() and (ratios["refracted"] <= 1.0).all() and tir_same.all()
    if name in ("floor", "depth bias"):
        assert plain.sum() >= 2900
    if name == "depth bias":          # every kept pixel lies on an instance with a depth bias, and R2 gives the frame's bits there too
        assert (tab["depthBias"][mine[kept]] != 0.0).all() and bit_equal[kept].all()
    assert (ratio_f[plain] <= 1.0).all()


# ---- 6. refusals and lifetime (R10) -----------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(rt64_lib, sample_data):
    """6.  R10: every refusal returns 0 with a message that names the function; count = 0 succeeds and touches nothing; K9's lifetime rules: RT64_SetMesh and
    RT64_DestroyMesh on a traced mesh and RT64_DestroyTexture on a texture of the frame refuse every call until the next frame."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    data, seed, options, flags = BC.make_case(sample_data, "floor")
    rays = np.ascontiguousarray(BC.rays_and_lods(data, "floor", seed, options)[0][:600])
    s = _open(rt64_lib, data)
    hip = ray_rule.Hip()
    R_ = rt64_lib
    try:
        n = len(rays)
        hits = np.zeros((n, 8), dtype=np.float32); out = np.full((8 * n, 8), 0xABABABAB, dtype=np.uint32); out2 = out.copy()
        d_rays, d_hits, d_out, d_out2, d_lods = hip.upload(rays), hip.upload(hits), hip.alloc(out.nbytes), hip.alloc(out.nbytes), hip.upload(np.zeros(n, dtype=np.float32))
        r, h_, o, o2 = rays.ctypes.data, hits.ctypes.data, out.ctypes.data, out2.ctypes.data
        Bh, Bd, Bt, Ch, Cd = ("RT64_BounceViewRayHits", "RT64_BounceViewRayHitsDevice", "RT64_TraceViewRayBounces", "RT64_TraceViewRayMirrorChains",
                              "RT64_TraceViewRayMirrorChainsDevice")

        def refused(word, fn, call):
            ok = call()
            assert ok == 0 and fn + ":" in R_.last_error() and word in R_.last_error(), (ok, R_.last_error())

        def all_refused(word):
            refused(word, Bh, lambda: R_.BounceViewRayHits(s.view, r, h_, None, o, None, None, n))
            refused(word, Bd, lambda: R_.BounceViewRayHitsDevice(s.view, d_rays, d_hits, None, d_out, None, None, 4, None))
            refused(word, Bt, lambda: R_.TraceViewRayBounces(s.view, r, None, None, o, None, None, n, 0))
            refused(word, Ch, lambda: R_.TraceViewRayMirrorChains(s.view, r, None, 2, o, o2, n, 0))
            refused(word, Cd, lambda: R_.TraceViewRayMirrorChainsDevice(s.view, d_rays, None, 2, d_out, d_out2, 4, 0, None))
        all_refused("draw")                                                               # before the first frame
        s.draw()
        assert R_.BounceViewRayHits(s.view, r, h_, None, o, None, None, 0) == 1
        assert R_.TraceViewRayBounces(s.view, r, None, None, o, None, None, 0, 0) == 1
        assert R_.TraceViewRayMirrorChains(s.view, r, None, 8, o, o2, 0, 0) == 1
        refused("NULL view", Bh, lambda: R_.BounceViewRayHits(None, r, h_, None, o, None, None, 4))
        refused("NULL", Bh, lambda: R_.BounceViewRayHits(s.view, None, h_, None, o, None, None, 4))
        refused("NULL", Bh, lambda: R_.BounceViewRayHits(s.view, r, None, None, o, None, None, 4))
        refused("all three output arrays are NULL", Bh, lambda: R_.BounceViewRayHits(s.view, r, h_, None, None, None, None, 4))
        refused("all three output arrays are NULL", Bd, lambda: R_.BounceViewRayHitsDevice(s.view, d_rays, d_hits, None, None, None, None, 4, None))
        refused("all three output arrays are NULL", Bt, lambda: R_.TraceViewRayBounces(s.view, r, None, None, None, None, None, 4, 0))
        refused("NULL", Ch, lambda: R_.TraceViewRayMirrorChains(s.view, r, None, 2, None, o2, 4, 0))
        refused("NULL", Ch, lambda: R_.TraceViewRayMirrorChains(s.view, r, None, 2, o, None, 4, 0))
        refused("unknown flags", Bt, lambda: R_.TraceViewRayBounces(s.view, r, None, None, o, None, None, 4, 0x4))
        refused("unknown flags", Ch, lambda: R_.TraceViewRayMirrorChains(s.view, r, None, 2, o, o2, 4, FIRST))
        refused("unknown flags", Cd, lambda: R_.TraceViewRayMirrorChainsDevice(s.view, d_rays, None, 2, d_out, d_out2, 4, 0x4, None))
        for depth in (0, 9, 0xFFFFFFFF):
            refused("depth must be 1 to 8", Ch, lambda: R_.TraceViewRayMirrorChains(s.view, r, None, depth, o, o2, 4, 0))
            refused("depth must be 1 to 8", Cd, lambda: R_.TraceViewRayMirrorChainsDevice(s.view, d_rays, None, depth, d_out, d_out2, 4, 0, None))
        for a, h, l, b, x, y in ((d_rays + 4, d_hits, None, d_out, None, None), (d_rays, d_hits + 8, None, d_out, None, None), (d_rays, d_hits, None, d_out + 4, None, None),
                                 (d_rays, d_hits, None, d_out, d_out2 + 8, None), (d_rays, d_hits, None, None, None, d_out2 + 4), (d_rays, d_hits, d_lods + 2, d_out, None, None)):
            refused("aligned", Bd, lambda: R_.BounceViewRayHitsDevice(s.view, a, h, l, b, x, y, 4, None))
        for a, l, b, x in ((d_rays + 4, None, d_out, d_out2), (d_rays, None, d_out + 8, d_out2), (d_rays, None, d_out, d_out2 + 4), (d_rays, d_lods + 1, d_out, d_out2)):
            refused("aligned", Cd, lambda: R_.TraceViewRayMirrorChainsDevice(s.view, a, l, 2, b, x, 4, 0, None))
        assert R_.BounceViewRayHitsDevice(s.view, d_rays, d_hits, d_lods + 4, d_out, None, None, 4, None) == 1          # lods need 4-byte alignment only
        assert (out == 0xABABABAB).all() and (out2 == 0xABABABAB).all()
        m = data.meshes[data.instances[1].mesh]
        s.set_mesh(s.meshes[data.instances[1].mesh], m.vertices, m.indices)
        all_refused("RT64_SetMesh")
        s.draw()
        assert R_.BounceViewRayHits(s.view, r, h_, None, o, None, None, 4) == 1, R_.last_error()
        # RT64_DestroyMesh on a mesh the frame traced (an extra instance of a mesh of its own, which goes first): refused until the next frame
        src = data.instances[1]
        far = np.array(src.transform, dtype=np.float32).copy(); far[3, 0] -= np.float32(30.0)
        mh = R_.CreateMesh(s.device, m.flags)
        s.set_mesh(mh, m.vertices, m.indices); s.meshes.append(mh)
        ih = R_.CreateInstance(s.scene); s.instances.append(ih)
        s.set_instance(len(s.instances) - 1, sample_scene.InstanceData("extra", len(s.meshes) - 1, far, far, src.diffuse, None, None, src.material))
        s.draw()
        R_.DestroyInstance(ih); s.instances.pop()
        R_.DestroyMesh(mh); s.meshes.pop()
        all_refused("mesh the view's last frame traced was destroyed")
        s.draw()
        assert R_.BounceViewRayHits(s.view, r, h_, None, o, None, None, 4) == 1, R_.last_error()
        # RT64_DestroyTexture of a texture the frame's table holds (a copy of a map on an extra instance, which goes first): K9's texture rule
        t = data.textures[6]
        td = rt64.TEXTURE_DESC(); buf, pitch = t.upload_buffer()
        td.bytes = buf.ctypes.data; td.byteCount = buf.nbytes; td.format = t.format; td.width, td.height, td.rowPitch = t.width, t.height, pitch
        th = R_.CreateTexture(s.device, td)
        assert th, R_.last_error()
        s.textures.append(th)
        ih = R_.CreateInstance(s.scene); s.instances.append(ih)
        s.set_instance(len(s.instances) - 1, sample_scene.InstanceData("extra", src.mesh, far, far, src.diffuse, None, len(s.textures) - 1, src.material))
        s.draw()
        R_.DestroyInstance(ih); s.instances.pop()
        R_.DestroyTexture(th); s.textures.pop()
        all_refused("texture of the view's last frame was destroyed")
        s.draw()
        assert R_.BounceViewRayHits(s.view, r, h_, None, o, None, None, 4) == 1, R_.last_error()
    finally:
        hip.close()
        s.close()


def test_an_enqueued_chain_outlives_the_mesh_it_walks(rt64_lib, sample_data):
    """7.  A chain enqueued on a caller's stream, then RT64_SetMesh on a mesh it walks: the call waits for the chain (Device::awaitQueries) before it rewrites the
    arrays, and the records are those of the frame."""
    from sm64rt_legacy_renderer_amd import rt64
    data, seed, options, flags = BC.make_case(sample_data, "facing")
    rays = BC.rays_and_lods(data, "facing", seed, options)[0]
    s = _open(rt64_lib, data, {"sync_present": 0})
    hip = ray_rule.Hip()
    try:
        s.draw()
        want_hits, want_rec = rt64.trace_view_ray_mirror_chains(rt64_lib, s.view, rays, 8)
        reps = 32
        many = np.ascontiguousarray(np.tile(rays, (reps, 1)))
        n = len(many)
        like = np.empty((8, n, 8), dtype=np.float32)
        d_rays, d_hits, d_rec = hip.upload(many), hip.alloc(like.nbytes), hip.alloc(like.nbytes)
        st = hip.stream()
        assert rt64_lib.TraceViewRayMirrorChainsDevice(s.view, d_rays, None, 8, d_hits, d_rec, n, 0, st) == 1, rt64_lib.last_error()
        k = next(i for i, inst in enumerate(data.instances) if inst.name == "sphere")
        m = data.meshes[data.instances[k].mesh]
        v = m.vertices.copy(); v["position"][:, :3] *= np.float32(0.5)
        s.set_mesh(s.meshes[data.instances[k].mesh], v, m.indices)
        got_hits = _bits(hip.download(d_hits, like)).reshape(8, reps, len(rays), 8); got_rec = _bits(hip.download(d_rec, like)).reshape(8, reps, len(rays), 8)
        assert (got_hits == _bits(want_hits)[:, None]).all() and (got_rec == _bits(want_rec)[:, None]).all()
        assert rt64_lib.TraceViewRayMirrorChains(s.view, rays.ctypes.data, None, 2, like.ctypes.data, like.ctypes.data, 4, 0) == 0 and "RT64_SetMesh" in rt64_lib.last_error()
    finally:
        hip.close()
        s.close()
