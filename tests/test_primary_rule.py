"""tests/primary_rule.py pinned on the CPU: hand-worked single pixels, the oracle's primary resolve held to the rule pixel by pixel and image by image in every case of
tests/primary_cases.py, and the named wrong variants of the rule, each of which must put the oracle outside the rule in the case built for it.

The bounds are the rule's; at most 0.5 % of a frame's pixels may be undecided (primary_cases.UNDECIDED_CAP)."""
import numpy as np
import pytest

import light_rule as L
import primary_cases as PC
import primary_rule as P

_sessions, _rules = {}, {}


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = PC.make_case(sample_data, name)
        _sessions[name] = (case, PC.oracle_session(case))
        _rules[name] = {}
    return _sessions[name]


# ---- hand-worked single pixels -------------------------------------------------------------------------------------------------------------------
# One camera for all of them: at the origin, looking down -z, fov 90 degrees, near 1, far 3, a 3 x 3 frame.  The projection is then x' = x, y' = y,
# z' = -1.5 z - 1.5, w' = -z, and the centre pixel (1, 1) has d = (1.5 / 3) 2 - 1 = 0: its ray is (0, 0, -1), NOT normalised but of length 1 here.

def _material(**over):
    m = dict(lightGroupMaskBits=1, ignoreNormalFactor=0.0, specularExponent=1.0, shadowRayBias=0.0, selfLight=(0.0, 0.0, 0.0), solidAlphaMultiplier=1.0,
             reflectionFactor=0.0, reflectionFresnelFactor=1.0, reflectionShineFactor=0.0, refractionFactor=0.0, fogEnabled=0, fogMul=1.0, fogOffset=0.0,
             fogColor=(0.0, 0.0, 0.0), depthBias=0.0, specularColor=(0.5, 0.25, 0.125), diffuseColorMix=(0.8, 0.4, 0.2, 1.0), lockMask=0.0)
    m.update(over)
    return m


def _facing(z, normal=(0.0, 0.0, 1.0), **material):
    """A triangle in the plane z = const around the axis, facing +z (e1 x e2 = (0, 0, 128))."""
    t = np.array([[[-8.0, -4.0, z], [8.0, -4.0, z], [0.0, 12.0, z]]])
    return dict(material=_material(**material), triangles=t, object_triangles=t, normals=np.tile(normal, (1, 3, 1)), transform=np.eye(4, dtype=np.float32),
                previousTransform=np.eye(4, dtype=np.float32), cull=True, texture=None)


def _scene(instances):
    return dict(instances=instances, lights=[], ambientBase=(0.25, 0.25, 0.25), ambientNoGI=(0.25, 0.25, 0.25), sky=[L.F(0.0)] * 3,
                bluenoise=np.zeros((512, 512, 4), dtype=np.uint8), frameCount=0, diSamples=0, shadow=L.BruteForceShadows([i["triangles"] for i in instances]))


def _camera(eye=(0.0, 0.0, 0.0), **over):
    view = np.eye(4, dtype=np.float32); view[3, :3] = -np.asarray(eye, dtype=np.float32)
    c = dict(view=view, fov=np.pi / 2.0, near=1.0, far=3.0, width=3, height=3, frameCount=1, canReproject=True, previous=None, upscaler=False, phases=8, background=None)
    c.update(over)
    return c


def _at(r, name, x=1, y=1):
    return r["images"][name][0][y, x]


def test_one_opaque_triangle_position_depth_and_flow_under_a_camera_translation():
    """The triangle z = -2 is met at t = 2: position (0, 0, -2); clip z = -1.5 * -2 - 1.5 = 1.5, w = 2: depth 0.75.  The previous camera stood at (0.5, 0, 0): there
    the point was at view x = -0.5, ndc -0.25, screen 0.375; now it is at screen 0.5.  flow = (0.5 - 0.375) * 3 = 0.375 px; FLOW stores (-x, y) = (-0.375, 0).
    Without canReproject the previous matrix is this frame's, and on the first frame as well: flow 0."""
    scene = _scene([_facing(-2.0)])
    r = P.primary(scene, _camera(previous=_camera(eye=(0.5, 0.0, 0.0))))
    assert r["decided"][1, 1] and r["id"][1, 1] == 0
    assert np.allclose(_at(r, "position"), [0.0, 0.0, -2.0], atol=1e-12) and np.allclose(_at(r, "depth"), 0.75, atol=1e-12)
    assert np.allclose(_at(r, "flow"), [-0.375, 0.0], atol=1e-12) and np.allclose(_at(r, "view"), [0.0, 0.0, -1.0], atol=1e-12)
    assert np.allclose(_at(r, "normal"), [0.0, 0.0, 1.0], atol=1e-12) and np.allclose(_at(r, "specular"), [0.5, 0.25, 0.125], atol=1e-12)
    assert r["images"]["flow"][1][1, 1].max() < 1e-3 and r["images"]["depth"][1][1, 1, 0] < 1e-4
    # colour (0.8, 0.4, 0.2) = (204, 102, 51) / 255, full coverage
    assert (r["diffuse_lo"][1, 1] <= [204, 102, 51, 255]).all() and (r["diffuse_hi"][1, 1] >= [204, 102, 51, 255]).all() and (r["diffuse_hi"][1, 1] - r["diffuse_lo"][1, 1] <= 1).all()
    for cam in (_camera(previous=_camera(eye=(0.5, 0.0, 0.0)), canReproject=False), _camera(previous=None)):
        assert np.array_equal(_at(P.primary(scene, cam), "flow"), [0.0, 0.0])
    # a pixel to the right, (2, 1): d = (2.5 / 3) 2 - 1 = 2 / 3, direction (2 / 3, 0, -1), position (4 / 3, 0, -2): t counts view-space depth, not length
    assert np.allclose(_at(r, "position", 2, 1), [4.0 / 3.0, 0.0, -2.0], atol=1e-12) and np.allclose(_at(r, "view", 2, 1), [2.0 / 3.0, 0.0, -1.0], atol=1e-12)


def test_a_miss():
    """(V12) Nothing is met: id -1, position 0, normal = -direction = (0, 0, 1), specular 0, depth 1, coverage 0.  The flow is that of the point 100000 down the ray:
    seen from (0.5, 0, 0) it stood at view x = -0.5, w = 100000: screen 0.5 - 0.25e-5; flow = 0.25e-5 * 3 = 7.5e-6, stored (-7.5e-6, 0)."""
    scene = _scene([_facing(2.0)])                                   # behind the camera
    r = P.primary(scene, _camera(previous=_camera(eye=(0.5, 0.0, 0.0))))
    assert r["decided"][1, 1] and r["id"][1, 1] == -1 and r["first"]["count"][1, 1] == 0
    assert np.array_equal(_at(r, "position"), [0.0, 0.0, 0.0]) and np.allclose(_at(r, "normal"), [0.0, 0.0, 1.0], atol=1e-12)
    assert np.array_equal(_at(r, "specular"), [0.0, 0.0, 0.0]) and _at(r, "depth")[0] == 1.0 and r["images"]["depth"][1][1, 1, 0] < 1e-6
    assert np.allclose(_at(r, "flow"), [-7.5e-6, 0.0], rtol=0, atol=1e-12)
    assert (r["diffuse_lo"][1, 1] == 0).all() and (r["diffuse_hi"][1, 1] == 0).all()


def test_two_panes_and_a_wall_coverage_and_the_first_storing_hit():
    """Front to back: an unlit pane (mask 0) of alpha 0.4 at t = 1.5, a lit pane of alpha 0.6 at t = 2, an opaque wall at t = 2.5.
    Pane 1 contributes 0.4 and stores nothing: TRANSPARENT = colour * 0.4 * ambient 0.5 = (0.16, 0.08, 0.04); coverage left 0.6.
    Pane 2 contributes 0.6 * 0.6 = 0.36, is lit above alpha 0.5 and is the FIRST storing hit: id 1, position (0, 0, -2), depth 0.75; coverage left 0.24.
    The wall contributes 0.24 with colour (0.2, 0.4, 0.8) and changes no state.  DIFFUSE = 0.36 (0.8, 0.4, 0.2) + 0.24 (0.2, 0.4, 0.8) = (0.336, 0.24, 0.264), alpha 1."""
    scene = _scene([_facing(-1.5, lightGroupMaskBits=0, solidAlphaMultiplier=0.4), _facing(-2.0, solidAlphaMultiplier=0.6), _facing(-2.5, diffuseColorMix=(0.2, 0.4, 0.8, 1.0))])
    r = P.primary(scene, _camera())
    assert r["decided"][1, 1] and r["id"][1, 1] == 1 and r["info"]["contributing"][1, 1] == 3 and r["info"]["storing_hit"][1, 1] == 1
    assert np.allclose(_at(r, "transparent"), [0.16, 0.08, 0.04], atol=1e-12) and np.allclose(_at(r, "reactive"), 0.16, atol=1e-12)
    assert np.allclose(_at(r, "position"), [0.0, 0.0, -2.0], atol=1e-12) and np.allclose(_at(r, "depth"), 0.75, atol=1e-12)
    want = np.rint(np.array([0.336, 0.24, 0.264, 1.0]) * 255.0)
    assert (r["diffuse_lo"][1, 1] <= want).all() and (r["diffuse_hi"][1, 1] >= want).all()
    # the wrong variants this pixel tells apart
    assert P.primary(scene, _camera(), mutate="state_last_hit")["id"][1, 1] == 2 and P.primary(scene, _camera(), mutate="state_from_unlit")["id"][1, 1] == 0
    # with a depth bias of 1.25 the wall is sorted first (2.5 - 1.25 < 1.5) and, opaque, ends the loop; it still lies at t = 2.5
    scene["instances"][2]["material"]["depthBias"] = 1.25
    r = P.primary(scene, _camera())
    assert r["id"][1, 1] == 2 and r["info"]["contributing"][1, 1] == 1 and np.allclose(_at(r, "position"), [0.0, 0.0, -2.5], atol=1e-12)
    assert np.allclose(_at(P.primary(scene, _camera(), mutate="depth_without_bias"), "position"), [0.0, 0.0, -1.25], atol=1e-12)


def test_a_mirror_fresnel_and_the_lock_sum():
    """A mirror (reflectionFactor 0.5, Fresnel factor 3, lockMask 0.25) whose normal is (0, 0.6, 0.8): 1 + n . d = 1 - 0.8 = 0.2, 0.2^5 = 0.00032,
    F = 0.5 + 0.5 * 0.00032 * 3 = 0.50048.  REFLECTION.a = F * 1; lock = 0.25 * 1 + F = 0.75048 -> 1 when binary; DIFFUSE = colour * (1 - F).
    A second mirror behind an alpha-0.6 first one: REFLECTION.a is ASSIGNED by the last mirroring hit, F * 0.4 (1 - F) * ... not the sum."""
    scene = _scene([_facing(-2.0, normal=(0.0, 0.6, 0.8), reflectionFactor=0.5, reflectionFresnelFactor=3.0, lockMask=0.25)])
    r = P.primary(scene, _camera())
    fres = 0.50048
    assert r["decided"][1, 1] and np.allclose(_at(r, "reflection_a"), fres, atol=1e-4) and r["images"]["reflection_a"][1][1, 1, 0] < 1e-3
    assert np.allclose(r["info"]["lock"][1, 1], 0.25 + fres, atol=1e-4) and _at(r, "lock")[0] == 1.0
    assert np.allclose(r["info"]["lock"][1, 1] - P.primary(scene, _camera(), mutate="lock_without_mirror_term")["info"]["lock"][1, 1], fres, atol=1e-4)
    want = np.rint(np.array([0.8, 0.4, 0.2]) * (1.0 - fres) * 255.0)
    assert (r["diffuse_lo"][1, 1, :3] <= want).all() and (r["diffuse_hi"][1, 1, :3] >= want).all() and (r["diffuse_hi"][1, 1] - r["diffuse_lo"][1, 1] <= 1).all()
    two = _scene([_facing(-1.5, normal=(0.0, 0.6, 0.8), reflectionFactor=0.5, reflectionFresnelFactor=3.0, solidAlphaMultiplier=0.6),
                  _facing(-2.0, normal=(0.0, 0.6, 0.8), reflectionFactor=0.5, reflectionFresnelFactor=3.0)])
    r = P.primary(two, _camera())
    assert np.allclose(_at(r, "reflection_a"), fres * 0.4, atol=1e-4) and r["id"][1, 1] == 0
    assert np.allclose(_at(P.primary(two, _camera(), mutate="reflect_alpha_summed"), "reflection_a"), fres * 0.6 + fres * 0.4, atol=1e-4)


def test_glass_zeroes_the_coverage_and_ends_the_loop():
    """Glass of alpha 0.6 (refractionFactor 0.9) before a wall: it contributes 0.6, is lit and stores; REFRACTION.a = the coverage left, 0.4; the coverage becomes 0,
    so the wall behind it adds nothing: DIFFUSE = 0.6 colour, alpha 1."""
    scene = _scene([_facing(-2.0, solidAlphaMultiplier=0.6, refractionFactor=0.9), _facing(-2.5, diffuseColorMix=(0.2, 0.4, 0.8, 1.0))])
    r = P.primary(scene, _camera())
    assert r["decided"][1, 1] and r["id"][1, 1] == 0 and r["info"]["contributing"][1, 1] == 1 and np.allclose(_at(r, "refraction_a"), 0.4, atol=1e-12)
    want = np.rint(np.array([0.48, 0.24, 0.12, 1.0]) * 255.0)
    assert (r["diffuse_lo"][1, 1] <= want).all() and (r["diffuse_hi"][1, 1] >= want).all()
    assert P.primary(scene, _camera(), mutate="glass_keeps_coverage")["info"]["contributing"][1, 1] == 2


def test_lock_binary_and_continuous_on_either_side_of_a_half():
    """lockMask 0.75 on a surface of alpha 0.6 gives 0.45: 0 as a step, 0.45 behind an upscaler; at alpha 1 it gives 0.75: 1 and 0.75.  A sum of exactly 0.5
    -- lockMask 0.5 at alpha 1 -- is a step no margin decides: LOCK alone is left open at that pixel."""
    for alpha, lock, step in ((0.6, 0.45, 0.0), (1.0, 0.75, 1.0)):
        scene = _scene([_facing(-2.0, solidAlphaMultiplier=alpha, lockMask=0.75)])
        r = P.primary(scene, _camera())
        assert r["lock_binary"] and r["lock_decided"][1, 1] and _at(r, "lock")[0] == step and np.allclose(r["info"]["lock"][1, 1], lock, atol=1e-12)
        r = P.primary(scene, _camera(upscaler=True, frameCount=0))
        assert not r["lock_binary"] and np.allclose(_at(r, "lock"), lock, atol=1e-12) and r["images"]["lock"][1][1, 1, 0] < 1.1 * 0.5 / 255.0
    r = P.primary(_scene([_facing(-2.0, lockMask=0.5)]), _camera())
    assert r["decided"][1, 1] and not r["lock_decided"][1, 1]


def test_jitter_is_halton_minus_a_half():
    """(V2) Frame 0 behind an upscaler of 8 phases: Halton(1, 2) - 0.5 = 0, Halton(1, 3) - 0.5 = -1 / 6; frame 2: (0.75, 1 / 9) - 0.5; frame 8 is frame 0 again."""
    j = lambda f: P.jitter(dict(upscaler=True, phases=8, frameCount=f))
    assert np.allclose(j(0), (0.0, 1.0 / 3.0 - 0.5), atol=1e-15) and np.allclose(j(2), (0.25, 1.0 / 9.0 - 0.5), atol=1e-15) and j(8) == j(0)
    assert P.jitter(dict(upscaler=False, phases=8, frameCount=2)) == (0.0, 0.0) and P.phase_count(88, 88) == 8 and P.phase_count(1920, 1280) == 18
    # the jitter moves the ray: at frame 2 the centre pixel has d = ((1.5 + 0.25) / 3) 2 - 1 = 1 / 6 in x
    r = P.primary(_scene([_facing(-2.0)]), _camera(upscaler=True, frameCount=2))
    assert np.allclose(_at(r, "view")[0], 1.0 / 6.0, atol=1e-12)


def test_background_uv_has_no_half_pixel():
    """(V14) screenUV of pixel (1, 1) of a 3 x 3 frame is (1 / 3, 1 / 3): u * 3 - 0.5 = 0.5, the even blend of texels 0 and 1 on both axes.  With red = 0, 60, 120 along x
    and green = 0, 90, 180 along y: (30, 45).  At the pixel's centre it would be texel (1, 1) itself: (60, 90)."""
    image = np.zeros((3, 3, 4), dtype=np.uint8); image[..., 0] = [0, 60, 120]; image[..., 1] = np.array([0, 90, 180])[:, None]; image[..., 3] = 255
    scene = _scene([_facing(2.0)])
    r = P.primary(scene, _camera(background=image))
    assert (r["diffuse_lo"][1, 1] <= [30, 45, 0, 0]).all() and (r["diffuse_hi"][1, 1] >= [30, 45, 0, 0]).all() and (r["diffuse_hi"][1, 1] - r["diffuse_lo"][1, 1] <= 1).all()
    r = P.primary(scene, _camera(background=image), mutate="background_uv_at_pixel_centre")
    assert (r["diffuse_lo"][1, 1, :2] == [60, 90]).all() and (r["diffuse_hi"][1, 1, :2] == [60, 90]).all()
    # pixel (0, 0): uv 0, the blend of texel 0 with the WRAPPED texel 2: (60, 90)
    r = P.primary(scene, _camera(background=image))
    assert (r["diffuse_lo"][0, 0, :2] <= [60, 90]).all() and (r["diffuse_hi"][0, 0, :2] >= [60, 90]).all()


# ---- the oracle, case by case --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PC.CASES)
def test_oracle_primary_resolve_within_the_rule(sample_data, oracle_lib, name):
    case, sess = _oracle(sample_data, oracle_lib, name)
    PC.hold(case, sess, "oracle", rules=_rules[name])


def test_the_case_tables_are_complete():
    assert set(PC.MUTATION_CASE) == set(P.MUTATIONS) and set(PC.MUTATION_CASE.values()) <= set(PC.CASES) and set(PC.SHARES) == set(PC.CASES)


@pytest.mark.parametrize("mutation", P.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put the oracle outside the rule in the case built to catch it (primary_cases.MUTATION_CASE), on more pixels than the case's compared frames
    leave undecided (with the right rule or with the wrong one)."""
    name = PC.MUTATION_CASE[mutation]
    case, sess = _oracle(sample_data, oracle_lib, name)
    rules = PC.rules_of(case, sess, _rules[name])
    bad = und_right = und_wrong = 0
    for f in case["compared"]:
        assert int(PC.judge(rules[f], sess[f])["bad"].sum()) == 0
        wrong = PC.run_rule(case, f, sess, mutate=mutation)
        bad += int(PC.judge(wrong, sess[f])["bad"].sum())
        und_right += int((~rules[f]["decided"]).sum()); und_wrong += int((~wrong["decided"]).sum())
    print("primary_rule mutation %-32s case %-16s bad=%d undecided=%d/%d" % (mutation, name, bad, und_wrong, und_right))
    assert bad > max(und_right, und_wrong), "the case built for %s, %s, does not tell it from the rule" % (mutation, name)
