"""`taa_upsample_kernel` held to tests/upscale_rule.py pixel by pixel (rules U1-U8).

A case of tests/upscale_cases.py draws at most 34 frames at a screen of at most 81 x 47 with the built-in upscaler.  For every compared frame N the rule predicts
UPSCALED from the GPU's own readbacks of frame N (OUTPUT_RGBA32F, FLOW, REACTIVE_MASK, LOCK_MASK, DEPTH), of frame N - 1 (UPSCALED), the sizes in RT64_FRAME_STATS and the
frame's index (the jitter is the rule's own Halton restatement): rgb must lie within the rule's own bound at every pixel, the count channel within its bound and exactly
1 on pixels without a history and 32 where the cap is certain, no pixel undecided or uncovered, and a frame behind a change of mode or display size starts over
everywhere.  Each case asserts from the rule's counts that it reaches what it was built for (upscale_cases.REACH).  The rule runs once per (case, frame, input bytes): a
launch form that stored the same inputs is held to the same result.

Launch forms: of test_gpu_temporal_rule.FORMS those that change what precedes or overlaps the pass on a frame with an upscaler -- `one-stream` and
`no-lds-cache` on `strafe`, and on `gi` the forms of the GI chain and the filter (`own-guide-and-input`, `plain-walk`).  A device that owns a band of rows refuses a
frame with an upscaler (the pass resamples across rows); the test asserts that refusal.  Nothing has been found outside the rule so far: no regression is recorded
here."""
import pytest

import upscale_cases as UC
import upscale_rule as UR
from test_gpu_temporal_rule import FORMS

pytestmark = pytest.mark.gpu

FORM_CASES = [("one-stream", "strafe"), ("no-lds-cache", "strafe"), ("own-guide-and-input", "gi"), ("plain-walk", "gi"), ("one-stream", "gi")]
_rules = {}


def _check(rt64_lib, sample_data, name, form):
    case = UC.make_case(sample_data, name)
    frames, stats = UC.gpu_session(rt64_lib, case, options=FORMS[form])
    side = "gpu/" + form
    for f in case["compared"]:
        st = stats[f]
        print("upscale_rule %-24s %-17s frame %2d fusedFrame=%d leanFrame=%d overlappedFrame=%d reflectionBesideDenoiser=%d render %dx%d screen %dx%d rows=%d..%d"
              % (side, name, f, st.fusedFrame, st.leanFrame, st.overlappedFrame, st.reflectionBesideDenoiser, st.width, st.height, st.screenWidth, st.screenHeight,
                 st.tileY0, st.tileY1))
        w, h = case["size_at"](f)
        assert (st.screenWidth, st.screenHeight) == (w, h) and (st.width, st.height) == UR.quality(case["mode_at"](f), w, h)[:2], (name, f, st.width, st.height)
        assert st.leanFrame == 0, (name, f)                                   # a frame with an upscaler is never lean (View::draw)
        if form == "one-stream":
            assert st.overlappedFrame == 0, (name, f)
    rows = UC.hold(case, frames, side, rules=_rules.setdefault(name, {}))
    return case, frames, rows


@pytest.mark.parametrize("name", UC.CASES + UC.GPU_ONLY_CASES)
def test_upscaled_within_the_rule(rt64_lib, sample_data, name):
    case, frames, _ = _check(rt64_lib, sample_data, name, "default")
    if name == "sharpened":
        # frame N is predicted from N - 1's UPSCALED: the history never sees the sharpened copy
        bad = [int(UR.compare(frames[n]["upscaled"], UC.run_rule(case, frames, n, mutate="history_is_sharpened"))["bad"].sum()) for n in case["compared"]]
        print("upscale_rule gpu %-32s %-17s bad=%s" % ("history_is_sharpened", name, bad))
        assert all(b > 0 for b in bad), bad


@pytest.mark.parametrize("form,name", FORM_CASES)
def test_upscaled_within_the_rule_on_every_launch_form(rt64_lib, sample_data, form, name):
    _check(rt64_lib, sample_data, name, form)


def test_a_band_refuses_a_frame_with_an_upscaler(rt64_lib, sample_data):
    """RT64_SetDeviceTile on a view with an upscaler: View::update refuses the frame (the pass reads rows of the whole frame), and says so."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    case = UC.make_case(sample_data, "strafe")
    s = sample_scene.Rt64Scene(rt64_lib, case["data_at"](0), *case["size_at"](0), hip_device=0)
    try:
        s.set_view_description(upscaler=rt64.UPSCALER_FSR, upscaler_mode=UR.MODE_QUALITY, **case["view"])
        s.set_tile(8, 24)
        s.draw()
        assert "need the whole frame on one device" in rt64_lib.last_error(), rt64_lib.last_error()
    finally:
        s.close()
