"""The kernels' GI temporal accumulation held to tests/temporal_rule.py pixel by pixel (rules N1-N8).

A case of tests/temporal_cases.py is a sequence of at most 71 frames of at most 88 x 72 drawn with GI and the denoiser on.  For every compared frame N a twin session
draws the same calls with denoiserEnabled = 0 on frame N alone: its INDIRECT_LIGHT_RAW and GI_MOMENTS are the fresh radiance, and the float64 rule predicts the
session's frame N from them, from the session's own frame N - 1 (INDIRECT_LIGHT_RAW, GI_MOMENTS, DEPTH, SHADING_NORMAL) and from FLOW, DEPTH, SHADING_NORMAL and
INSTANCE_ID of frame N.  INDIRECT_LIGHT_RAW (rgb and the history length in alpha) and GI_MOMENTS must lie within the rule's own bound at every pixel; the twin
conditions of N8 are checked on every run; DIRECT_LIGHT_RAW carries no history; the twin's INDIRECT_LIGHT_FILTERED is its INDIRECT_LIGHT_RAW.  The rule runs once per
(case, frame, input bytes): a launch form that stored the same inputs is held to the same result.

Both kernels that carry the accumulation are reached: `bounce_resolve_kernel` (the wavefront chain of all-opaque frames: every case but `layers`, behind each of
the chain's walks -- plain (bounce_split 0), two-phase, refill -- and grids) and `indirect_kernel<true>` (`layers`: per-pixel hit lists).  launch_indirect sends an
all-opaque frame with GI to the chain whatever bounce_split says (View::draw allocates the chain's records for it), so `indirect_kernel<false>` is not what
bounce_split 0 runs: no frame with GI samples reaches that instantiation.  Nothing has been found outside the rule so far: no regression is recorded here."""
import numpy as np
import pytest

import temporal_cases as TC

pytestmark = pytest.mark.gpu

# RT64_FRAME_STATS says which frame form ran (fusedFrame: 2 = the one-kernel primary + direct of an all-opaque frame, the frames whose GI is the wavefront chain; 0 with a
# translucent instance), whether the frame overlapped its predecessor (overlappedFrame: these sessions wait for every frame, so it is 0 with either value of
# overlap_frames and the option can only be required to be accepted), whether the reflection launches ran beside the filter
# (reflectionBesideDenoiser: 0 here, max_reflections is 0) and the rows a device owns (tileY0, tileY1).  It has no field for the walk a bounce trace took, its
# workgroup count, the LDS scene cache or who wrote the filter's guide and input: for those the test requires that the option was accepted.
FORMS = {
    "default": None, "plain-walk": {"bounce_split": 0}, "split-walk": {"bounce_split": 1}, "refill": {"bounce_refill": 1},
    "two-workgroups": {"bounce_groups": 2}, "no-lds-cache": {"lds_cache": 0}, "own-guide-and-input": {"fold_guide": 0, "fold_variance": 0},
    "reflection-in-line": {"overlap_reflection": 0}, "one-stream": {"overlap_frames": 0},
}
FORM_CASES = [("plain-walk", "static"), ("plain-walk", "strafe-left"), ("split-walk", "strafe-left"), ("refill", "strafe-left"),
              ("two-workgroups", "strafe-left"), ("no-lds-cache", "strafe-right"), ("own-guide-and-input", "turning"), ("reflection-in-line", "strafe-left"),
              ("one-stream", "strafe-left")]
BAND = (19, 53)
_rules = {}


def _check(rt64_lib, sample_data, name, form, band=None):
    case = TC.make_case(sample_data, name)
    stats = {}
    sessions = TC.gpu_session(rt64_lib, case, options=FORMS[form], band=band, stats=stats)
    side = "gpu/" + form + ("/band" if band else "")
    for f in case["compared"]:
        st = stats[f]
        print("temporal_rule %-22s %-13s frame %2d fusedFrame=%d leanFrame=%d overlappedFrame=%d reflectionBesideDenoiser=%d rows=%d..%d"
              % (side, name, f, st.fusedFrame, st.leanFrame, st.overlappedFrame, st.reflectionBesideDenoiser, st.tileY0, st.tileY1))
        assert st.fusedFrame == (0 if name == "layers" else 2) and st.leanFrame == 0 and st.reflectionBesideDenoiser == 0, (name, form, f, st.fusedFrame, st.leanFrame)
        assert band or (st.tileY0, st.tileY1) == (0, case["size"][1]), (name, form, f, st.tileY0, st.tileY1)
        if form == "one-stream":
            assert st.overlappedFrame == 0, (name, f)
    if band:
        # the band is held on its own rows: no previous row may leave it (a sideways strafe has no flow in y at all)
        for f in case["compared"]:
            flow = np.asarray(sessions[f]["a"]["flow"])
            assert flow.shape[0] == band[1] - band[0] and (flow[..., 1] == 0.0).all(), (name, f, "a previous row leaves the band")
    return TC.hold(case, sessions, side, rules=_rules.setdefault((name, band), {}), shares=band is None)


@pytest.mark.parametrize("name", TC.CASES)
def test_accumulation_within_the_rule(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "default")


@pytest.mark.parametrize("form,name", FORM_CASES)
def test_accumulation_within_the_rule_on_every_launch_form(rt64_lib, sample_data, form, name):
    _check(rt64_lib, sample_data, name, form)


def test_a_band_is_held_on_its_own_rows(rt64_lib, sample_data):
    """A device that owns rows 19..53 (set_tile): its readbacks are those rows, and the rule runs on them alone."""
    _check(rt64_lib, sample_data, "strafe-left", "default", band=BAND)
