"""The kernels' GI bounce held to tests/gi_rule.py pixel by pixel, per sample (rules I1-I12).

A case of tests/gi_cases.py is one session of two or three 88 x 72 frames drawn with max_reflections = 0 and the denoiser off.  What IndirectRayGen reads --
SHADING_POSITION, SHADING_NORMAL, INSTANCE_ID as stored, IMAGE_BACKGROUND where there is one -- goes through the float64 rule, and INDIRECT_LIGHT_RAW (rgb) and
GI_MOMENTS must lie within the rule's own bound at every pixel the rule decides; alpha is giSamples on a surface and 0 elsewhere, exactly; INDIRECT_LIGHT_FILTERED is
INDIRECT_LIGHT_RAW byte for byte; at most 0.5 % of a frame's surface pixels may be undecided.  The rule runs once per (case, frame): a launch form whose stored
inputs are the same bytes is held to the same result.

The all-opaque cases run the wavefront chain (bounce_trace_* -> bounce_hit -> bounce_miss -> bounce_resolve) in each of its forms; `layers` and `two-bounce-layers`
the one-kernel form with per-ray hit lists, also on the general build of the kernels and without the LDS scene cache."""
import pytest

import gi_cases as GC

pytestmark = pytest.mark.gpu

# Which of the two forms ran is read from RT64_FRAME_STATS.fusedFrame: 2 = the frame's primary and direct passes ran as the one kernel that serves frames whose
# instances are ALL provably opaque -- the frames whose GI is the wavefront chain; 0 on a frame with a translucent instance (per-pixel hit lists, indirect_kernel), and
# with fused_lean = 0.  RT64_FRAME_STATS has no field for the walk a bounce trace took, the LDS scene cache, the build of the kernels or the number of workgroups (see
# tests/test_gpu_light_rule.py): for these paths the test requires that the option was accepted.  bounce_groups = 4: the frame's 30 tiles on 4 workgroups, the
# several-tiles-per-workgroup walk.
PATHS = {"default": None, "refill": {"bounce_refill": 1}, "split": {"bounce_split": 1}, "plain": {"bounce_split": 0}, "no-lds-cache": {"lds_cache": 0},
         "general-kernels": {"simple_kernels": 0}, "four-workgroups": {"bounce_groups": 4}, "three-kernel-frame": {"fused_lean": 0}}
OPAQUE = [c for c in GC.CASES if c.startswith("opaque-")] + ["two-bounce-opaque"]
_rules = {}


def _check(rt64_lib, sample_data, name, path):
    case = GC.make_case(sample_data, name)
    stats = {}
    images = GC.gpu_session(rt64_lib, case, options=PATHS[path], stats=stats)
    opaque = name in OPAQUE or name in ("self-lit", "background", "sky-strength")
    for f, st in stats.items():
        assert st.fusedFrame == (2 if opaque and path != "three-kernel-frame" else 0), (name, path, f, st.fusedFrame)
    GC.hold(case, images, "gpu/" + path, rules=_rules.setdefault(name, {}))


@pytest.mark.parametrize("name", GC.CASES)
def test_gi_bounce_within_the_rule(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "default")


@pytest.mark.parametrize("path", [p for p in PATHS if p != "default"])
@pytest.mark.parametrize("name", OPAQUE)
def test_wavefront_chain_within_the_rule_on_every_launch_form(rt64_lib, sample_data, name, path):
    _check(rt64_lib, sample_data, name, path)


@pytest.mark.parametrize("path", ["general-kernels", "no-lds-cache"])
@pytest.mark.parametrize("name", ["layers", "two-bounce-layers"])
def test_one_kernel_form_within_the_rule_on_the_other_kernels(rt64_lib, sample_data, name, path):
    _check(rt64_lib, sample_data, name, path)
