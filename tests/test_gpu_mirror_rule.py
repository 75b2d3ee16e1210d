"""The kernels' reflection passes and refraction pass held to tests/mirror_rule.py pixel by pixel, per pass (rules M1-M12 and G1-G6).

Session k of a case is drawn with the device option max_reflections = k (tests/mirror_cases.py): what pass k reads -- SHADING_POSITION, VIEW_DIRECTION, SHADING_NORMAL,
INSTANCE_ID and REFLECTION as session k stores them, the continuation state folded in by the readback -- goes through the float64 rule, and session k + 1's REFLECTION,
folded state and "goes on" must be the rule's at every pixel the rule decides; REFRACTION likewise from session 0.  The images no pass writes are the same bytes in
every session, a pixel no pass takes keeps its G-buffer bytes, and the frame's reflectionRays / refractionRays are the pixels the passes take.  At most 0.5 % of the
pixels a pass takes may be undecided.  `floor`, `facing` and `glass` also run without the LDS scene cache, on the general build of the kernels and with the passes
launched on the aux stream beside the SVGF denoiser; `translucent`, `sky` (the per-pixel hit list) and `textured` also on the general build."""
import numpy as np
import pytest

import mirror_cases as MC

pytestmark = pytest.mark.gpu

# RT64_FRAME_STATS has no field for the LDS scene cache, the build of the kernels or the stream a pass ran on (see tests/test_gpu_light_rule.py): for these paths the
# test requires that the option was accepted.
PATHS = {"default": (None, None), "no-lds-cache": ({"lds_cache": 0}, None), "general-kernels": ({"simple_kernels": 0}, None),
         "aux-stream": ({"overlap_reflection": 1, "denoiser_mode": 1}, {"gi_samples": 1, "denoiser": True})}
_default = {}


def _inputs_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in MC.STATE + ("reflection",))


def _check(rt64_lib, sample_data, name, path):
    case = MC.make_case(sample_data, name)
    if name not in _default:
        sess, rays = MC.gpu_sessions(rt64_lib, case)
        _default[name] = (sess, rays, {})
    sess, rays, rules = _default[name]
    if path != "default":
        options, view = PATHS[path]
        base_sess, base_rules = sess, rules
        sess, rays = MC.gpu_sessions(rt64_lib, case, options=options, view=view)
        for f in case["compared"]:          # the same G-buffer on every path, byte for byte
            assert _inputs_equal(sess[(0, f)], base_sess[(0, f)])
        # the rule's result is reused for every pass whose inputs are the bytes the default path stored
        rules = {(f, k): r for (f, k), r in base_rules.items() if _inputs_equal(sess[(0 if k == "glass" else k, f)], base_sess[(0 if k == "glass" else k, f)])}
    MC.hold(case, sess, rays, "gpu/" + path, rules=rules, images_only=(path == "aux-stream"))
    return case, sess, rays, rules


@pytest.mark.parametrize("name", MC.CASES)
def test_mirror_and_glass_within_the_rule(rt64_lib, sample_data, name):
    case, sess, rays, rules = _check(rt64_lib, sample_data, name, "default")
    if name == "lone-pixel":                # pass 1 has work on under 1 % of the mirrored pixels, its twin on none: that launch takes the early-out and counts no ray
        on = int(rules[(0, 0)]["goes_on"].sum()); assert 0 < on < 0.01 * int(rules[(0, 0)]["takes"].sum()), on
    if name == "lone-pixel-none":
        assert not rules[(0, 0)]["goes_on"].any() and rays[(2, 0)][0] == rays[(1, 0)][0]
    if name == "facing":
        assert rules[(0, 4)]["takes"].sum() > 50
    if name == "frames":
        on = {f: int(rules[(f, 0)]["goes_on"].sum()) for f in case["compared"]}
        assert on[1] > 0 and on[4] > 0 and on[6] > 0 and on[3] == 0, on


@pytest.mark.parametrize("path", [p for p in PATHS if p != "default"])
@pytest.mark.parametrize("name", ["floor", "facing", "glass"])
def test_mirror_and_glass_within_the_rule_on_every_launch_form(rt64_lib, sample_data, name, path):
    _check(rt64_lib, sample_data, name, path)


@pytest.mark.parametrize("name", ["translucent", "textured", "sky"])
def test_hit_lists_and_texels_within_the_rule_on_the_general_kernels(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "general-kernels")
