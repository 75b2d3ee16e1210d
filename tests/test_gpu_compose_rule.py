"""The kernels' ComposePS held to tests/compose_rule.py pixel by pixel (rules C1-C6).

A case of tests/post_cases.py draws at most three frames of at most 64 x 40 and reads back at most eight images of the last one.  The float64 rule predicts
OUTPUT_RGBA32F from DIFFUSE, the two filtered light images and REFLECTION, REFRACTION and TRANSPARENT -- on a lean frame from DIFFUSE, DIRECT_LIGHT_RAW and the scene's
two ambient colours -- and every channel must lie within the rule's own bound; FINAL_RGBA8 must lie in the UNORM8 interval of value +- bound and, where the launch that
stored OUTPUT stored the back buffer too, be the conversion of the stored float32 byte for byte.  The rule runs once per (case, input bytes): a launch form that read the
same inputs is held to the same result.

Every restatement of the pass is reached: `compose_pixel` of svgf.hip (`plain`: the fold into the last a-trous iteration), `compose_post_kernel<false>` as its own launch
(`plain` with fold_compose 0, `gaussian`, `cutout`), `compose_lean_value` inside lean_frame_kernel (`lean`: it stores the back buffer; OUTPUT is materialised on readback
by `compose_post_kernel<true>`, so each image is held to the rule on its own) and `compose_lean_pixel` inside direct_kernel (`lean` with fused_lean 0).  Nothing has been
found outside the rule so far: no regression is recorded here."""
import pytest

import post_cases as PCS

pytestmark = pytest.mark.gpu

# RT64_FRAME_STATS says whether the frame was lean (leanFrame) and which kernel form drew it (fusedFrame: 1 = the one-kernel lean frame, 2 = the one-kernel primary +
# direct of an all-opaque full frame, 0 = separate kernels).  It has no field for where ComposePS ran on a full frame: fold_compose can only be required to be accepted.
# (case, form) -> (device options, leanFrame, fusedFrame, one launch stores OUTPUT and the back buffer)
FORMS = {
    ("plain", "default"): (None, 0, 0, True), ("plain", "own-compose"): ({"fold_compose": 0}, 0, 0, True),
    ("lean", "default"): (None, 1, 1, False), ("lean", "three-kernel"): ({"fused_lean": 0}, 1, 0, True),
    ("gaussian", "default"): (None, 0, 2, True), ("gaussian", "separate-kernels"): ({"fused_lean": 0}, 0, 0, True),
    ("cutout", "default"): (None, 0, 0, True),
}
_rules = {}


@pytest.mark.parametrize("name,form", sorted(FORMS))
def test_compose_within_the_rule(rt64_lib, sample_data, name, form):
    options, lean, fused, same_launch = FORMS[(name, form)]
    case = PCS.make_case(sample_data, name)
    img, st = PCS.gpu_session(rt64_lib, case, options=options)
    print("compose_rule gpu/%-14s %-10s leanFrame=%d fusedFrame=%d %dx%d" % (form, name, st.leanFrame, st.fusedFrame, st.width, st.height))
    assert (st.leanFrame, st.fusedFrame) == (lean, fused) and bool(st.leanFrame) == case["lean"], (name, form, st.leanFrame, st.fusedFrame)
    assert (st.width, st.height, st.screenWidth, st.screenHeight) == case["size"] * 2
    PCS.hold_compose(case, img, "gpu/" + form, rules=_rules.setdefault(name, {}), same_launch=same_launch)


def test_back_buffer_of_a_primary_spp_frame_is_the_conversion_of_its_output(rt64_lib, sample_data):
    """primary_spp = 2: the sub-frames' outputs cannot be read back, so their mean stays with the oracle parity tests; what is held here is that the back buffer is the
    UNORM8 conversion of the stored mean, byte for byte (spp_accumulate_kernel stores both)."""
    import compose_rule as CR
    case = PCS.make_case(sample_data, "spp")
    img, st = PCS.gpu_session(rt64_lib, case)
    assert st.leanFrame == 0 and img["final"].shape == img["output"].shape
    assert (img["final"] == CR.unorm8_of_float32(img["output"])).all() and (img["final"][..., 3] == 255).all()
