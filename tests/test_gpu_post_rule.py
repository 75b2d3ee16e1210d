"""`post_process_kernel` held to tests/post_rule.py pixel by pixel (rules X1-X8).

A case of tests/post_cases.py draws at most three frames at a screen of at most 81 x 48 and reads back at most five images of the last one.  The float64 rule predicts
the back buffer from the GPU's own readback of the image PostProcessPS samples (OUTPUT_RGBA32F; UPSCALED behind the upscaler; SHARPENED with a sharpness), FLOW, the
sizes, the blur's strength and sample count and the first ray-traced instance's rectangles: inside the rectangles every channel of FINAL_RGBA8 must lie in the UNORM8
interval of the rule's value +- its own bound, outside them the bytes must be what the frame had before the pass -- (0, 0, 0, 255), or BACKGROUND's rgb under a
background instance.  Each case asserts from the rule's counts that it reaches the edge it was built for (post_cases.REACH).  The rule runs once per (case, input
bytes).  Nothing has been found outside the rule so far: no regression is recorded here."""
import pytest

import post_cases as PCS

pytestmark = pytest.mark.gpu

_rules = {}


@pytest.mark.parametrize("name", PCS.POST_CASES + PCS.GPU_ONLY_POST_CASES)
def test_back_buffer_within_the_rule(rt64_lib, sample_data, name):
    case = PCS.make_case(sample_data, name)
    img, st = PCS.gpu_session(rt64_lib, case)
    print("post_rule gpu %-15s leanFrame=%d fusedFrame=%d render %dx%d screen %dx%d" % (name, st.leanFrame, st.fusedFrame, st.width, st.height, st.screenWidth, st.screenHeight))
    assert (st.screenWidth, st.screenHeight) == case["size"] and (case["render"] is None or (st.width, st.height) == case["render"]), (name, st.width, st.height)
    # RT64_FRAME_STATS has no field for the separate post pass; a frame with motion blur is never lean, one with an upscaler neither (View::draw)
    if case["view"].get("motion_blur", 0.0) > 0.0 or case["view"].get("upscaler", 0):
        assert st.leanFrame == 0
    if case["source"] != "output":
        assert (st.width, st.height) != case["size"]          # the quality mode renders below the screen size: the source is not the render-size output
    PCS.hold_post(case, img, "gpu", rules=_rules.setdefault(name, {}))
