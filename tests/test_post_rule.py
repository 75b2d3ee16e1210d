"""tests/post_rule.py pinned on the CPU: hand-made 4 x 3 and 5 x 2 images whose every texel has its own value, one test per sentence of the rule; the oracle's
PostProcessPS (`pass_post`) held to the rule pixel by pixel in every case of tests/post_cases.py it can draw; and the named wrong variants of the rule, each of which
must put the oracle outside the rule in the case built to catch it.

The asserted conditions are the rule's: every byte inside the rectangles within the UNORM8 interval of value +- bound (ratio < 1), no pixel
uncovered, every byte outside them equal to the buffer before the pass.  MIN_BAD states for each variant at least how many pixels leave it: half of what the oracle
shows (profiles/compose_post_rule_deviation.txt); the variants of the rectangles are geometry: their counts are stated as the
geometry gives them and at least nine tenths must show."""
import numpy as np
import pytest

import post_cases as PCS
import post_rule as PR
from light_rule import F

_sessions = {}
MIN_BAD = {"clamp_not_wrap": 116, "no_half_texel": 1597, "taps_not_clamped": 180, "start_not_halved": 1257, "flow_in_pixels": 1594, "step_over_samples_minus_one": 835,
           "flow_nearest_at_screen_size": 293, "uv_over_screen_not_viewport": 283}
# The variants of the rectangles are geometry: (pixels inside the variant's rectangles that leave it, pixels outside them that differ) as the oracle shows them.
# rect: scissor x 12..41, y 19..38 (600 pixels).  Not flipped it is y 9..28: rows 9..18 are black where the variant expects the picture, rows 19..28 hold another part of
# it (600 together), and the 300 pixels of rows 29..38 are outside for the variant and not black.  Inclusive edges add column 42 and row 39: 20 + 30 + 1 pixels that are
# black.  rect-background: 12 columns of 48 rows on the left.  (A pixel of the picture that happened to be black would lower a count by one: the counts hold on the
# oracle's images of these cases, which are flat colours and a sky.)
GEOMETRY_BAD = {"rect_not_flipped": (600, 300), "scissor_inclusive": (51, 0), "outside_left_black_over_background": (0, 576)}


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = PCS.make_case(sample_data, name)
        _sessions[name] = (case, PCS.oracle_session(case))
    return _sessions[name]


# ---- hand-made images ---------------------------------------------------------------------------------------------------------------------------------

def _image(w=4, h=3):
    """Every texel its own value, multiples of 1 / 64 in [0, 1): red 8 x + y, green 8 y + x, blue x + 5 y + 1 (over 64)."""
    x, y = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    return np.stack([(8 * x + y) / 64.0, (8 * y + x) / 64.0, (x + 5 * y + 1) / 64.0, np.ones((h, w))], axis=-1).astype(np.float32)


def _flow(w, h, fx=0.0, fy=0.0):
    return np.broadcast_to(np.array([fx, fy], dtype=np.float32), (h, w, 2)).copy()


def _run(src, screen, flow=None, strength=0.0, samples=32, **kw):
    h, w = src.shape[:2]
    return PR.post_process(src, _flow(w, h) if flow is None else flow, screen, (w, h), strength, samples, **kw)


def test_a_texel_centre_returns_the_texel():
    """The half texel (X4): at the source's own size uv x size - 0.5 is the pixel's index and the weights are 0.  Without it every pixel is a blend with three neighbours."""
    for size in ((4, 3), (5, 2)):
        src = _image(*size)
        r = _run(src, size)
        assert np.abs(r["value"] - src[..., :3]).max() < 1e-7 and r["inside"].all() and r["covered"].all()
        assert (r["lo"][..., :3] <= PR.CR.unorm8(src[..., :3])).all() and (PR.CR.unorm8(src[..., :3]) <= r["hi"][..., :3]).all() and (r["lo"][..., 3] == 255).all()
        wrong = _run(src, size, mutate="no_half_texel")
        blend = 0.25 * (src[:, :, :3] + np.roll(src, -1, axis=1)[..., :3] + np.roll(src, -1, axis=0)[..., :3] + np.roll(np.roll(src, -1, axis=0), -1, axis=1)[..., :3])
        assert np.abs(wrong["value"] - blend).max() < 1e-7


def test_wrap_on_each_of_the_four_sides():
    """4 x 3 shown at 8 x 6: texel = (x + 0.5) / 2 - 0.5.  Column 0 is at -0.25: a quarter of the LAST column; column 7 at 3.25: a quarter of the FIRST.  Rows likewise."""
    src = _image(); s = src[..., :3].astype(np.float64)
    r = _run(src, (8, 6))
    v = r["value"]
    assert np.abs(v[0, 0] - (0.5625 * s[0, 0] + 0.1875 * s[0, 3] + 0.1875 * s[2, 0] + 0.0625 * s[2, 3])).max() < 1e-7          # left and top
    assert np.abs(v[5, 7] - (0.5625 * s[2, 3] + 0.1875 * s[2, 0] + 0.1875 * s[0, 3] + 0.0625 * s[0, 0])).max() < 1e-7          # right and bottom
    assert np.abs(v[2, 0] - (0.75 * (0.25 * s[0, 0] + 0.75 * s[1, 0]) + 0.25 * (0.25 * s[0, 3] + 0.75 * s[1, 3]))).max() < 1e-7  # left only: texel row 0.75
    assert np.abs(v[0, 3] - (0.75 * (0.75 * s[0, 1] + 0.25 * s[0, 2]) + 0.25 * (0.75 * s[2, 1] + 0.25 * s[2, 2]))).max() < 1e-7  # top only: texel column 1.25
    c = r["info"]["counts"]
    assert (c["wrapped_left"], c["wrapped_right"], c["wrapped_top"], c["wrapped_bottom"]) == (6, 6, 8, 8)
    clamped = _run(src, (8, 6), mutate="clamp_not_wrap")["value"]
    assert np.abs(clamped[0, 0] - s[0, 0]).max() < 1e-7 and np.abs(clamped[5, 7] - s[2, 3]).max() < 1e-7
    # the bound there carries the coordinate's error times the difference between the two ends of the row, which WRAP makes neighbours
    # (red: 24 / 64 between columns 3 and 0, 8 / 64 between columns 0 and 1)
    assert (r["bound"][:, 0, 0] > r["bound"][:, 2, 0]).all()


def test_taps_at_u_0_and_u_1_blend_the_last_column_with_the_first():
    src = _image(5, 2); s = src[..., :3].astype(np.float64)
    for u in (0.0, 1.0):
        val, info = PR.sample(s, F(np.array([u, u])), F(np.array([0.25, 0.75])))          # v: the centres of the two rows
        got = np.stack([c.v for c in val], axis=-1)
        assert np.abs(got - 0.5 * (s[:, 4] + s[:, 0])).max() < 1e-12 and info["edge_blend"].all()
        assert info["wrapped_left"].all() if u == 0.0 else info["wrapped_right"].all()
    val, info = PR.sample(s, F(np.array([0.5])), F(np.array([1.0])))                       # v = 1: half the last row, half the first; u = 0.5 is the centre of column 2
    assert np.abs(np.stack([c.v for c in val], axis=-1) - 0.5 * (s[1, 2] + s[0, 2])).max() < 1e-12 and info["wrapped_bottom"].all()


def test_the_threshold_just_above_just_below_and_inside_the_margin():
    """flow / resolution against 1e-6f (X7), on a uniform flow: 4 x 3 render size, so flow.x = 4e-6 is the threshold itself."""
    src = _image()
    above = _run(src, (4, 3), flow=_flow(4, 3, fx=4.5e-6), strength=1.0)
    assert above["blurred"].all() and not above["near_threshold"].any() and above["info"]["counts"]["blurred"] == 12
    below = _run(src, (4, 3), flow=_flow(4, 3, fx=3.5e-6), strength=1.0)
    assert not below["blurred"].any() and not below["near_threshold"].any()
    assert (below["value"] == _run(src, (4, 3))["value"]).all()
    at = _run(src, (4, 3), flow=_flow(4, 3, fx=float(np.float32(4.0) * np.float32(1e-6))), strength=1.0)
    assert at["near_threshold"].all() and at["info"]["counts"]["near_threshold"] == 12
    # inside the margin a pixel is held to both branches: the interval contains the plain sample's and the blurred mean's
    plain = _run(src, (4, 3))
    assert (at["lo"] <= plain["lo"]).all() and (at["hi"] >= plain["hi"]).all()
    # the length is that of both components
    diag = _run(src, (4, 3), flow=_flow(4, 3, fx=3.0e-6, fy=2.5e-6), strength=1.0)         # 0.75e-6 and 0.83e-6: each under the threshold, together 1.12e-6
    assert diag["blurred"].all()
    assert not _run(src, (4, 3), flow=_flow(4, 3, fx=1.0), strength=0.0)["blurred"].any() and not _run(src, (4, 3), flow=_flow(4, 3, fx=1.0), strength=1.0, samples=0)["blurred"].any()


def test_one_sample_is_the_start_of_the_gather_and_two_are_its_mean_with_the_centre():
    """A flow of one pixel to the right in a 4 x 3 frame is 0.25 in uv.  samples = 1: the one tap is uv - flow x strength / 2, half a texel to the left: the mean of
    the pixel and its left neighbour, and at column 0 the tap is clamped to u = 0: the last column and the first.  samples = 2 adds the tap at uv itself."""
    src = _image(); s = src[..., :3].astype(np.float64)
    one = _run(src, (4, 3), flow=_flow(4, 3, fx=1.0), strength=1.0, samples=1)
    half = 0.5 * (s + np.roll(s, 1, axis=1))
    assert one["blurred"].all() and np.abs(one["value"] - half).max() < 1e-7
    two = _run(src, (4, 3), flow=_flow(4, 3, fx=1.0), strength=1.0, samples=2)
    assert np.abs(two["value"] - 0.5 * (half + s)).max() < 1e-7
    assert np.abs(_run(src, (4, 3), flow=_flow(4, 3, fx=1.0), strength=1.0, samples=2, mutate="step_over_samples_minus_one")["value"][:, 1:3]
                  - 0.5 * (half + 0.5 * (s + np.roll(s, -1, axis=1)))[:, 1:3]).max() < 1e-7
    assert np.abs(_run(src, (4, 3), flow=_flow(4, 3, fx=1.0), strength=1.0, samples=1, mutate="start_not_halved")["value"][:, 1:] - np.roll(s, 1, axis=1)[:, 1:]).max() < 1e-7
    # strength 3, one sample: the tap is a texel and a half to the left; columns 0 and 1 leave the frame and are clamped to u = 0
    far = _run(src, (4, 3), flow=_flow(4, 3, fx=1.0), strength=3.0, samples=1)
    edge = 0.5 * (s[:, 3] + s[:, 0])
    assert np.abs(far["value"][:, 0] - edge).max() < 1e-7 and np.abs(far["value"][:, 1] - edge).max() < 1e-7 and np.abs(far["value"][:, 2] - 0.5 * (s[:, 0] + s[:, 1])).max() < 1e-7
    assert far["info"]["counts"]["clamped_left"] == 3 and far["info"]["counts"]["edge_blend"] == 6
    loose = _run(src, (4, 3), flow=_flow(4, 3, fx=1.0), strength=3.0, samples=1, mutate="taps_not_clamped")
    assert np.abs(loose["value"][:, 0] - 0.5 * (s[:, 2] + s[:, 3])).max() < 1e-7           # unclamped it wraps a whole texel further
    # a flow in pixels that is not divided by the resolution is four times as long
    assert np.abs(_run(src, (4, 3), flow=_flow(4, 3, fx=0.25), strength=1.0, samples=1, mutate="flow_in_pixels")["value"] - half).max() < 1e-7


def test_rectangles_flip_exclusive_edges_and_zero_size():
    """Screen 8 x 6.  RT64_RECT (2, 1, 3, 2) from the bottom-left is columns 2..4, rows 3..4 from the top (X1, X2)."""
    src = _image()
    r = _run(src, (8, 6), scissor=(2, 1, 3, 2))
    want = np.zeros((6, 8), dtype=bool); want[3:5, 2:5] = True
    assert np.array_equal(r["inside"], want) and r["scissor"] == (2, 3, 5, 5) and r["viewport"] == (0, 0, 8, 6)
    assert (r["lo"][~want] == PR.CLEAR).all() and (r["hi"][~want] == PR.CLEAR).all() and r["info"]["counts"]["outside_rectangle"] == 42
    assert np.array_equal(r["value"], _run(src, (8, 6))["value"])                           # a scissor moves no uv
    wrong = _run(src, (8, 6), scissor=(2, 1, 3, 2), mutate="rect_not_flipped")["inside"]
    unflipped = np.zeros((6, 8), dtype=bool); unflipped[1:3, 2:5] = True
    assert np.array_equal(wrong, unflipped)
    incl = np.zeros((6, 8), dtype=bool); incl[3:6, 2:6] = True
    assert np.array_equal(_run(src, (8, 6), scissor=(2, 1, 3, 2), mutate="scissor_inclusive")["inside"], incl)
    # a viewport of the source's own size: uv runs over the VIEWPORT, so its pixels are the texels
    v = _run(src, (8, 6), viewport=(2, 1, 4, 3))
    inside = np.zeros((6, 8), dtype=bool); inside[2:5, 2:6] = True
    assert np.array_equal(v["inside"], inside) and v["viewport"] == (2, 2, 4, 3) and np.abs(v["value"][2:5, 2:6] - src[..., :3]).max() < 1e-7
    over_screen = _run(src, (8, 6), viewport=(2, 1, 4, 3), mutate="uv_over_screen_not_viewport")
    assert np.abs(over_screen["value"][2:5, 2:6] - _run(src, (8, 6))["value"][2:5, 2:6]).max() < 1e-12
    # both: the intersection
    both = _run(src, (8, 6), viewport=(2, 1, 4, 3), scissor=(0, 0, 4, 3))
    want = np.zeros((6, 8), dtype=bool); want[3:5, 2:4] = True
    assert np.array_equal(both["inside"], want)
    # a rectangle without a width or a height is not set: the screen
    for rect in ((2, 1, 0, 2), (2, 1, 3, 0), (0, 0, 0, 0), None):
        z = _run(src, (8, 6), scissor=rect, viewport=rect)
        assert z["inside"].all() and z["scissor"] == (0, 0, 8, 6) and z["viewport"] == (0, 0, 8, 6)
    # outside, the buffer before the pass: its rgb with alpha 255
    before = np.zeros((6, 8, 4), dtype=np.uint8); before[..., 0] = np.arange(8) + 1; before[..., 1] = (np.arange(6) + 1)[:, None]
    b = _run(src, (8, 6), scissor=(2, 1, 3, 2), before=before)
    assert (b["lo"][~b["inside"]][:, :3] == before[~b["inside"]][:, :3]).all() and (b["lo"][..., 3] == 255).all() and np.array_equal(b["lo"][~b["inside"]], b["hi"][~b["inside"]])
    black = _run(src, (8, 6), scissor=(2, 1, 3, 2), before=before, mutate="outside_left_black_over_background")
    assert (black["lo"][:, :2, :3] == 0).all() and (black["lo"][:, 5:, :3] == before[:, 5:, :3]).all()
    stored = b["lo"].copy()
    c = PR.compare(stored, b)
    assert (c["bad"], c["outside_bad"]) == (0, 0)
    stored[0, 0, 0] += 1; stored[3, 2, 1] = stored[3, 2, 1] + 2
    c = PR.compare(stored, b)
    assert (c["bad"], c["outside_bad"]) == (1, 1) and c["ratio"][0] > 1.0


def test_a_value_that_is_not_finite_is_not_covered():
    src = _image(); src[1, 2, 1] = np.inf
    with np.errstate(invalid="ignore"):
        r = _run(src, (8, 6))
    assert r["info"]["counts"]["not_covered"] > 0 and PR.compare(r["lo"], r)["bad"] == r["info"]["counts"]["not_covered"]
    assert _run(_image(), (8, 6))["info"]["counts"]["not_covered"] == 0


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PCS.POST_CASES)
def test_oracle_back_buffer_within_the_rule(sample_data, oracle_lib, name):
    case, img = _oracle(sample_data, oracle_lib, name)
    PCS.hold_post(case, img, "oracle")


@pytest.mark.parametrize("mutation", PR.MUTATIONS)
def test_wrong_variant_puts_the_oracle_outside_the_rule(sample_data, oracle_lib, mutation):
    name = PCS.POST_MUTATION_CASE[mutation]
    case, img = _oracle(sample_data, oracle_lib, name)
    c = PR.compare(img["final"], PCS.run_post(case, img, mutate=mutation))
    print("post_rule oracle %-36s %-15s bad=%d outside_bad=%d" % (mutation, name, c["bad"], c["outside_bad"]))
    if mutation in GEOMETRY_BAD:
        # never more than the geometry gives, and at least nine tenths of it
        for got, most in zip((c["bad"], c["outside_bad"]), GEOMETRY_BAD[mutation]):
            assert most * 9 // 10 <= got <= most and (got > 0 or most == 0), (mutation, c["bad"], c["outside_bad"])
    else:
        assert c["bad"] >= MIN_BAD[mutation], (mutation, c["bad"])
