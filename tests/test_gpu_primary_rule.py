"""The kernels' primary resolve held to tests/primary_rule.py pixel by pixel and image by image (rules V1-V14).

A case of tests/primary_cases.py is one session of a few 88 x 72 frames drawn with max_reflections = 0.  The rule reads the scene and the cameras, never a stored
image (but IMAGE_BACKGROUND for the background term), so its result per (case, frame) is computed once and every launch form is held to the same one:
SHADING_POSITION, SHADING_NORMAL, SHADING_SPECULAR, TRANSPARENT, FLOW, REACTIVE_MASK, LOCK_MASK, DEPTH, VIEW_DIRECTION and the alphas of REFLECTION and REFRACTION
within the rule's bound, DIFFUSE among the bytes the rule's interval allows, INSTANCE_ID, FIRST_INSTANCE_ID and the binary LOCK_MASK equal, the first entry of the
rule's hit list the stored PRIMARY_HIT record, at every pixel the rule decides; at most 0.5 % of a frame's pixels may be undecided.

`static`, `camera` and `movers` run on every launch form of the frame; `layers`, `translucent-lit` and `mirror-glass` (the per-pixel hit list, the transparent-light
draw) also on the general build of the kernels and without the LDS scene cache."""
import pytest

import primary_cases as PC

pytestmark = pytest.mark.gpu

GI = {"gi_samples": 1, "denoiser": True}
# path -> (device options, view-description overrides, (leanFrame, fusedFrame) the frame statistics must report, or None).  RT64_FRAME_STATS has no field for the
# LDS scene cache, the build of the kernels or the number of workgroups (see tests/test_gpu_light_rule.py): for those paths the test requires that the option was
# accepted.  `lean-frame` is the default path of an all-opaque scene without GI: the one-kernel frame that stores the back buffer only, every other image coming
# from View::materialise on readback (a new transform or camera keeps a frame lean); the other cases' default path is whatever form the library picks for them.
PATHS = {"default": (None, None, None), "lean-frame": (None, None, (1, 1)), "full-frame": ({"lean_frames": 0}, None, (0, 2)),
         "gi-one-kernel": ({"fused_lean": 1}, GI, (0, 2)), "gi-three-kernels": ({"fused_lean": 0}, GI, (0, 0)),
         "no-lds-cache": ({"lds_cache": 0}, None, None), "general-kernels": ({"simple_kernels": 0}, None, None), "four-workgroups": ({"max_frame_groups": 4}, None, None)}
_rules = {}


def _check(rt64_lib, sample_data, name, path):
    case = PC.make_case(sample_data, name)
    options, view, form = PATHS[path]
    stats = {}
    images = PC.gpu_session(rt64_lib, case, options=options, view=view, stats=stats)
    for f, st in stats.items():
        print("primary_rule %-22s %-16s frame %d leanFrame=%d fusedFrame=%d" % ("gpu/" + path, name, f, st.leanFrame, st.fusedFrame))
        if form is not None:
            assert st.leanFrame == form[0] and form[1] in (None, st.fusedFrame), (path, name, f, st.leanFrame, st.fusedFrame)
    PC.hold(case, images, "gpu/" + path, rules=_rules.setdefault(name, {}))


@pytest.mark.parametrize("name", PC.CASES)
def test_primary_resolve_within_the_rule(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "default")


@pytest.mark.parametrize("path", [p for p in PATHS if p != "default"])
@pytest.mark.parametrize("name", ["static", "camera", "movers"])
def test_primary_resolve_within_the_rule_on_every_launch_form(rt64_lib, sample_data, name, path):
    _check(rt64_lib, sample_data, name, path)


@pytest.mark.parametrize("path", ["general-kernels", "no-lds-cache"])
@pytest.mark.parametrize("name", ["layers", "translucent-lit", "mirror-glass"])
def test_hit_lists_and_the_transparent_light_within_the_rule_on_the_other_kernels(rt64_lib, sample_data, name, path):
    _check(rt64_lib, sample_data, name, path)
