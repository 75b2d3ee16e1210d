"""tests/lighting_rule.py pinned on the CPU.  No CPU path produces lighting records, so the rule is pinned to the picture instead (P8): for every case of
tests/lighting_cases.py the oracle draws a frame with di_samples = 0 and max_lights = 16, the rule's core is evaluated at the frame's stored G-buffer with the
float64 camera direction, and direct + emitted is held against the oracle's DIRECT_LIGHT_RAW within L8, and -- on the scenes whose casters are all opaque --
against light_rule.direct_light's own value within the sum of both errors.  Then the rule itself: every case keeps its shares and its undecided cap, every named
wrong variant leaves the bound of the right rule on its case, and hand-worked records give the numbers one can do on paper.
"""
import ctypes as C

import numpy as np
import pytest

import light_cases as LC
import light_rule
import lighting_cases as PC
import lighting_rule as R
import material_cases as MC
import material_rule as M

LEFT_OUT_CAP = 0.005          # L9's cap: pixels left out of the comparison with the picture, of the shaded ones
_frames, _rules = {}, {}


def _camera(data, w, h):
    return dict(view=np.asarray(data.view, dtype=np.float64), fov=float(np.float32(data.fov)), near=float(np.float32(data.near)), far=float(np.float32(data.far)),
                width=w, height=h, jitter=(0.0, 0.0))


def _oracle_frame(sample_data, name):
    """(scene, width, height, frameCount, the oracle's frame) of lighting_cases.picture_case."""
    if name not in _frames:
        from oracle import oracle_py
        d, w, h, frames = PC.picture_case(sample_data, name)
        o = oracle_py.OracleScene(d)
        try:
            for f in range(frames):
                ref = o.render(w, h, images=(f == frames - 1), diSamples=0, maxLights=16)
        finally:
            o.close()
        assert ref["pixelJitter"] == (0.0, 0.0)
        _frames[name] = (d, w, h, frames - 1, ref)
    return _frames[name]


def _case_rule(sample_data, name, mutate=None):
    """The rule on the case's own rays and the oracle's hits of them; the unmutated one once per case."""
    if mutate is None and name in _rules:
        return _rules[name]
    data, seed, options, heights = PC.make_case(sample_data, name)
    rays, lods = PC.rays_and_lods(data, seed, options, heights)
    key = ("hits", name)
    if key not in _rules:
        _rules[key] = PC.oracle_hits(data, rays)
    rule = R.lighting(data, M.texture_levels(data, MC.mipmapped(options)), rays, _rules[key], lods, mutate=mutate)
    if mutate is None:
        _rules[name] = rule
    return rule


# ---- against the picture (P8) ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PC.NAMES)
def test_the_rule_gives_the_oracles_direct_light(sample_data, oracle_lib, name):
    d, w, h, frame_count, ref = _oracle_frame(sample_data, name)
    cam = _camera(d, w, h)
    value, bound, decided, info = R.at_gbuffer(d, M.texture_levels(d), ref["shadingPosition"], ref["shadingNormal"], ref["shadingSpecular"], ref["instanceId"], cam)
    lit = ref["instanceId"] >= 0
    # which pixels the picture itself decides, and draws every candidate once: light_rule's evaluation of the same frame.  Its shadows take every caster for
    # opaque, so its VALUE is the picture's only where no caster is translucent; its candidate counts, draws and CDF decisions hold everywhere, and a shadow ray
    # it cannot decide grazes a triangle whatever that triangle's alpha is.
    r = LC.rule_inputs(d)
    r["camera"] = cam
    shadow = light_rule.BruteForceShadows(r["triangles"])
    lv, lb, ldec, linfo = light_rule.direct_light(ref["shadingPosition"], ref["shadingNormal"], ref["shadingSpecular"], ref["instanceId"], r["materials"], r["lights"],
                                                  r["eye_diffuse"], r["eye_specular"], 16, 0, frame_count, d.bluenoise, r["camera"], shadow)
    opaque_scene = name in PC.FROM_LIGHT_CASES or name == "mipped maps"
    once = linfo["draws"] == linfo["candidates"]
    held = lit & decided & once & ldec
    assert np.array_equal(info["admitted"][lit], linfo["candidates"][lit])
    dev = np.abs(ref["directLight"][..., :3].astype(np.float64) - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(dev == 0.0, 0.0, dev / bound).max(axis=-1)
    left_out = 1.0 - held.sum() / lit.sum()
    both = 0.0
    if opaque_scene:          # the two float64 statements agree within the sum of their errors
        with np.errstate(divide="ignore", invalid="ignore"):
            pair = np.abs(lv[..., :3] - value) / (lb[..., :3] + bound)
        both = float(pair.max(axis=-1)[held].max())
    print("lighting_rule oracle %-24s shaded %4d held %4d left out %.4f  ratio max %.4f mean %.5f  against light_rule %.4f  blocked somewhere %.3f  two or more lights %.3f" %
          (name, int(lit.sum()), int(held.sum()), left_out, ratio[held].max(), ratio[held].mean(), both, (info["blocked"][lit] > 0).mean(), (info["admitted"][lit] >= 2).mean()))
    assert lit.sum() >= 150 and left_out <= LEFT_OUT_CAP, left_out          # (the veils leave few pixels with an opaque surface at all)
    assert (ratio[held] < 1.0).all(), float(ratio[held].max())
    assert both < 1.0


# ---- the rule itself --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PC.NAMES)
def test_every_case_is_worth_running(sample_data, oracle_lib, name):
    rule = _case_rule(sample_data, name)
    sh = R.shares(rule)
    real = int((rule["kind"] == 2).sum())
    print("lighting_rule case %-24s hits %4d  in shadow %.3f  two or more lights %.3f  through a layer %.3f  unlit %.3f  truncated %.3f  undecided %.4f %s" %
          ((name, real) + sh + (rule["why"],)))
    assert real >= 400
    assert all(a >= b for a, b in zip(sh[:5], PC.SHARES[name])), (sh, PC.SHARES[name])
    assert sh[5] <= PC.UNDECIDED_CAP
    # the records the rule would store pass its own comparison: the float32 rounding of a value is inside its bound
    ratios, exact = R.compare(rule, R.as_records(rule))
    assert exact.all() and all((r <= 0.51).all() for r in ratios.values())


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put the right rule's records outside its bound on more records than either leaves undecided."""
    name = PC.MUTATION_CASE[mutation]
    right = _case_rule(sample_data, name)
    wrong = _case_rule(sample_data, name, mutate=mutation)
    ratios, exact = R.compare(wrong, R.as_records(right))
    out = ~exact
    for r in ratios.values():
        out |= ~(r <= 1.0)
    und = int((wrong["undecided"] | right["undecided"]).sum())
    print("lighting_rule mutation %-28s case %-12s outside=%d undecided=%d" % (mutation, name, int(out.sum()), und))
    assert out.sum() > und


def _hand_scene(sample_data, shadow_offset=0.0, occluder=True, mask=0xFFFFFFFF):
    """small_sample without its maps (normal (0, 1, 0), specular 1); the floor's second triangle at u = 0.25, v = 0.5 is the point (3.75, 0, 5); one light 5 away
    at (3.75, 4, 8), direction (0, 0.8, 0.6); a 1.5 x 1.5 opaque quad half way, around (3.5, 2, 6.25)."""
    from sm64rt_legacy_renderer_amd import rt64
    d = MC.small_sample(sample_data)
    d.shader_flags = rt64.SHADER_RASTER_ENABLED | rt64.SHADER_RAYTRACE_ENABLED
    d.instances = list(d.instances); d.meshes = list(d.meshes)
    floor = d.instances[3]
    floor.material.specularExponent = 2.0; floor.material.selfLight = rt64.VECTOR3(0.01, 0.02, 0.03); floor.material.lightGroupMaskBits = mask
    desc = type(d.desc)(); C.memmove(C.byref(desc), C.byref(d.desc), C.sizeof(desc)); d.desc = desc          # (never the session's sample scene)
    d.desc.eyeLightDiffuseColor = rt64.VECTOR3(0.1, 0.1, 0.1); d.desc.eyeLightSpecularColor = rt64.VECTOR3(0.2, 0.2, 0.2)
    d.lights = [LC._light(sample_data.lights[0], (3.75, 4.0, 8.0), (1.0, 0.5, 0.25), radius=10.0, exponent=2.0, shadow_offset=shadow_offset, spec=(1.0, 1.0, 1.0))]
    if occluder:
        LC._add_quad(d, (3.5, 2.0, 6.25))          # (the ray crosses it a quarter unit off its centre: not on the diagonal its two triangles share)
    return d


def _hand_record(d, instance=1, prim=1):
    rays = np.zeros((1, 8), dtype=np.float32); rays[0, 0:3] = (3.75, 5.0, 5.0); rays[0, 4:7] = (0.0, -1.0, 0.0); rays[0, 7] = np.inf
    hits = np.zeros((1, 8), dtype=np.float32); hits[0, 0:3] = (5.0, 0.25, 0.5)
    hits.view(np.int32)[0, 3] = instance; hits.view(np.uint32)[0, 4] = prim
    rule = R.lighting(d, M.texture_levels(d), rays, hits)
    assert not rule["undecided"].any()
    for k in ("direct", "unshadowed", "emitted"):
        assert (rule[k][1] < 1e-5).all()
    return rule


def test_hand_worked_records(sample_data):
    # falloff (1 - 5 / 10)^2 = 0.25; N.L = 0.8: Lambert 0.2; reflect(-L, N) = (0, 0.8, -0.6), . -rayDirection (0, 1, 0) = 0.8, x 0.25 = 0.2, ^2 = 0.04, x specular 1:
    # term = (1, 0.5, 0.25) x 0.2 + (1, 1, 1) x 0.04.  Self light (0.01, 0.02, 0.03); eye light: N . -rayDirection = 1, reflect(rayDirection, N) . -rayDirection = 1:
    # 0.1 + 0.2 in every channel.
    term, emitted = np.array([0.24, 0.14, 0.09]), np.array([0.31, 0.32, 0.33])
    close = lambda a, b: np.allclose(a, b, rtol=0, atol=1e-7)          # (the colours are float32 numbers: 0.1 is 0.100000001)
    lit = _hand_record(_hand_scene(sample_data, occluder=False))
    assert lit["kind"][0] == 2 and lit["flags"][0] == R.VALID and lit["admitted"][0] == 1 and lit["blocked"][0] == 0 and lit["walks"][0] == 1
    assert close(lit["direct"][0][0], term) and close(lit["unshadowed"][0][0], term) and close(lit["emitted"][0][0], emitted)
    shadowed = _hand_record(_hand_scene(sample_data))                                       # the quad at t = 2.5 of 5
    assert shadowed["admitted"][0] == 1 and shadowed["blocked"][0] == 1 and shadowed["flags"][0] == R.VALID
    assert close(shadowed["direct"][0][0], 0.0) and close(shadowed["unshadowed"][0][0], term) and close(shadowed["emitted"][0][0], emitted)
    short = _hand_record(_hand_scene(sample_data, shadow_offset=3.0))                       # tMax = 5 - 3 = 2: the ray ends in front of the quad
    assert short["blocked"][0] == 0 and short["walks"][0] == 1 and close(short["direct"][0][0], term)
    inside = _hand_record(_hand_scene(sample_data, shadow_offset=5.0))                      # tMax = 0 < tMin = 0.1: Q6-invalid, visibility 1, no walk
    assert inside["blocked"][0] == 0 and inside["walks"][0] == 0 and inside["admitted"][0] == 1 and close(inside["direct"][0][0], term)
    unlit = _hand_record(_hand_scene(sample_data, mask=0))
    assert unlit["flags"][0] == R.VALID | R.UNLIT and unlit["admitted"][0] == 0 and unlit["walks"][0] == 0
    assert close(unlit["direct"][0][0], 0.0) and close(unlit["unshadowed"][0][0], 0.0) and close(unlit["emitted"][0][0], emitted)
    # from below: the back face, the normal flipped to (0, -1, 0) -- the light is behind it: N.L = -0.8 + 0.707 < 0, not admitted
    d = _hand_scene(sample_data, occluder=False)
    rays = np.zeros((1, 8), dtype=np.float32); rays[0, 0:3] = (3.75, -5.0, 5.0); rays[0, 4:7] = (0.0, 1.0, 0.0); rays[0, 7] = np.inf
    hits = np.zeros((1, 8), dtype=np.float32); hits[0, 0:3] = (5.0, 0.25, 0.5); hits.view(np.int32)[0, 3] = 1; hits.view(np.uint32)[0, 4] = 1
    back = R.lighting(d, M.texture_levels(d), rays, hits)
    assert back["flags"][0] == R.VALID | R.BACK_FACE and back["admitted"][0] == 0 and close(back["emitted"][0][0], emitted)
    # a miss and two bad hits: P1's records
    d = _hand_scene(sample_data)
    for instance, prim, flags in ((-1, 0, 0), (99, 0, R.BAD_HIT), (1, 2, R.BAD_HIT)):
        rule = _hand_record(d, instance, prim)
        rec = R.as_records(rule).view(np.uint32)[0]
        assert rule["kind"][0] == (0 if instance < 0 else 1)
        assert rec[3] == flags and rec[12] == 0xFFFFFFFF and rec[13] == 0xFFFFFFFF and not rec[[0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15]].any()
