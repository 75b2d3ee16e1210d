"""tests/raster_rule.py pinned on the CPU: hand-worked pixels, the oracle's rasteriser (oracle/oracle_raster.c) held to the rule pixel by pixel in every case of
tests/raster_cases.py -- FINAL_RGBA8 and BACKGROUND, coverage and byte intervals -- and the named wrong variants of the rule, each of which must put the oracle
outside the rule in the case built for it while the right rule has no pixel outside.

The share of undecided pixels depends on the rule and the inputs alone: at most 1 % of a frame's pixels (raster_cases.UNDECIDED_CAP), none in the exact cases."""
import numpy as np
import pytest

import raster_cases as RC
import raster_rule as R

_sessions = {}


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = RC.make_case(sample_data, name)
        _sessions[name] = (case, RC.oracle_images(case), RC.run_rule(case))
    return _sessions[name]


# ---- hand-worked pixels --------------------------------------------------------------------------------------------------------------------------
# A 4 x 4 frame whose viewport is the frame: NDC x = -1 + px / 2, y = 1 - py / 2; the centre of pixel (1, 2) is NDC (-0.25, -0.25).

VC = RC.SHADER_VERTEX_COLOUR


def _instance(pos, colours, **over):
    inst = dict(pos=np.array(pos, dtype=np.float64), indices=np.arange(len(pos)), inputs=[np.array(colours, dtype=np.float64)], uv=None, shader_id=VC, filter=1,
                haddr=0, vaddr=0, levels=None, viewport=None, scissor=None, background=False)
    inst.update(over)
    return inst


def _draw(insts, target=None, **kw):
    return R.draw(np.zeros((4, 4, 4), dtype=np.uint8) if target is None else target, insts, 4, 4, **kw)


def test_rect_origin_is_bottom_left():
    """RT64_RECT (1, 0, 2, 1) of a frame 4 high: columns 1..2 of the BOTTOM row, which is row 3 of the pixel grid."""
    assert R.rect_pixels((1, 0, 2, 1), 4) == (1, 3, 3, 4) and R.rect_pixels((1, 0, 2, 1), 4, top_left=True) == (1, 0, 3, 1)


def test_top_left_rule_on_a_pixel_grid_aligned_quad():
    """Two triangles that share the diagonal of the square NDC [-0.75, 0.25]^2 = pixels [0.5, 2.5]^2: its corners are pixel centres, every step exact.  Centres on the
    left and top edges belong to it, those on the right and bottom edges do not; the shared diagonal is covered exactly once: pixels (0..1, 0..1), alpha 0.6 -> 153."""
    a, b, c, d = (-0.75, 0.75, 0.5, 1.0), (0.25, 0.75, 0.5, 1.0), (0.25, -0.25, 0.5, 1.0), (-0.75, -0.25, 0.5, 1.0)
    col = [(1.0, 0.4, 0.2, 0.6)] * 6
    r = _draw([_instance([a, b, c, a, c, d], col)])
    want = np.zeros((4, 4), dtype=np.int64); want[0:2, 0:2] = 1
    assert np.array_equal(r["layers"], want) and not r["undecided"].any() and r["counts"]["exact_triangles"] == 2 and r["counts"]["ties"] >= 7
    assert (r["lo"][0, 0] == [153, 61, 31, 153]).all() and (r["hi"][0, 0] == [153, 61, 31, 153]).all()
    # the other orientation of both: the same pixels
    assert np.array_equal(_draw([_instance([a, c, b, a, d, c], col)])["layers"], want)
    wrong = np.zeros((4, 4), dtype=np.int64); wrong[1:3, 1:3] = 1
    assert np.array_equal(_draw([_instance([a, b, c, a, c, d], col)], mutate="bottom_right_rule")["layers"], wrong)


def test_perspective_correct_colour_and_its_affine_variant():
    """An edge from w = 1 (red 0) to w = 3 (red 1) seen at its screen midpoint: clip-space weight of the far end is (1/2 / 3) / (1/2 / 1 + 1/2 / 3) = 1/4, not 1/2.
    The triangle NDC (-1, 1), (1, 1), (-1, -3) covers the centre of pixel (1, 0), NDC (-0.25, 0.75): screen barycentrics (0.5625, 0.375, 0.0625) of w (1, 3, 1):
    weights / w = (0.5625, 0.125, 0.0625) -> 1/6 of the far corner: red = 1/6, alpha 1 -> byte 42.5: 42 or 43."""
    pos = [(-1.0, 1.0, 0.5, 1.0), (3.0, 3.0, 1.5, 3.0), (-1.0, -3.0, 0.5, 1.0)]
    col = [(0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0)]
    r = _draw([_instance(pos, col)])
    assert r["layers"][0, 1] == 1 and not r["undecided"][0, 1]
    mid = 0.5 * (r["flo"][0, 1, 0] + r["fhi"][0, 1, 0])
    assert abs(mid - 1.0 / 6.0) < 1e-4 and r["lo"][0, 1, 0] <= 42 and r["hi"][0, 1, 0] >= 43 and r["hi"][0, 1, 0] - r["lo"][0, 1, 0] <= 1
    a = _draw([_instance(pos, col)], mutate="affine_attributes")
    assert abs(0.5 * (a["flo"][0, 1, 0] + a["fhi"][0, 1, 0]) - 0.375) < 1e-4


def test_depth_range_w_and_the_guard_band_without_a_clipper():
    """A triangle that covers the frame with z / w running from -1 at the left edge of NDC to +1 at the right (z = x): z < 0 left of the middle -> columns 0, 1 are
    outside, 2, 3 inside.  With z = x + 0.5 w: z > w right of NDC 0.5 -> column 3 is outside as well as column 0.  The guard band on screen.  With a corner behind the eye
    the part in front of it is drawn."""
    col = [(1.0, 1.0, 1.0, 1.0)] * 3
    tri = lambda zf: [(-1.0, 1.0, zf(-1.0), 1.0), (3.0, 1.0, zf(3.0), 1.0), (-1.0, -3.0, zf(-1.0), 1.0)]
    r = _draw([_instance(tri(lambda x: x), col)])
    assert np.array_equal(r["layers"], np.tile([0, 0, 1, 1], (4, 1))) and not r["undecided"].any()
    assert _draw([_instance(tri(lambda x: x), col)], mutate="near_plane_ignored")["layers"].all()
    r = _draw([_instance(tri(lambda x: x + 0.5), col)])                       # z / w = x + 0.5 at the centres -0.75, -0.25, 0.25, 0.75: -0.25, 0.25, 0.75, 1.25
    assert np.array_equal(r["layers"], np.tile([0, 1, 1, 0], (4, 1)))
    assert np.array_equal(_draw([_instance(tri(lambda x: x + 0.5), col)], mutate="far_plane_ignored")["layers"], np.tile([0, 1, 1, 1], (4, 1)))
    # the guard band: a 1 x 1 viewport at pixel (1, 1) puts NDC +-4 two pixels either side of x = 1.5, y = 1.5 -> x in (-0.5, 3.5): column 3 (centre 3.5) is on the line
    big = [(-9.0, 9.0, 0.5, 1.0), (27.0, 9.0, 0.5, 1.0), (-9.0, -27.0, 0.5, 1.0)]
    r = _draw([_instance(big, col, viewport=(1, 2, 1, 1))])
    assert r["undecided"][:, 3].all() and r["undecided"][3, :].all() and r["layers"][0:3, 0:3].all()
    # behind the eye: A = NDC (-1, -1) and B = (1, -1) in front (w = 1, z = 0.5), C = clip (0, 1, 0.5, -1) behind.  The points a A + b B + c C with w = a + b - c > 0:
    # x / w = (b - a) / w, y / w = (c - a - b) / w = -1: EVERY visible point projects onto the line y = -1 -- the triangle is seen edge-on and covers no pixel centre
    r = _draw([_instance([(-1.0, -1.0, 0.5, 1.0), (1.0, -1.0, 0.5, 1.0), (0.0, 1.0, 0.5, -1.0)], col)])
    assert not r["layers"].any()
    # A = (-1, 1), B = (1, 1) in front, C = clip (0, -3, 0.25, -1) behind (it would project to (0, 3), ABOVE the edge AB).  With s = a + b: y / w = (s - 3 c) / (s - c)
    # = 1 - 2 c / (s - c) <= 1: what is in front of the eye lies BELOW AB, on the side away from C's projection.  The centre of pixel (1, 3), NDC (-0.25, -0.75), is
    # a = 1.0625, b = 0.8125, c = 0.875 (w = 1), z = 0.25 (a + b + c) = 0.6875 <= w: covered.  z <= w ends the piece where c = 0.6 s, at y / w = -2, below the frame.
    r = _draw([_instance([(-1.0, 1.0, 0.25, 1.0), (1.0, 1.0, 0.25, 1.0), (0.0, -3.0, 0.25, -1.0)], col)])
    assert r["counts"]["behind_one"] > 0 and r["layers"][3, 1] == 1 and r["layers"][3, 2] == 1 and r["layers"][0, 1] == 1


def test_blend_through_the_stored_byte():
    """Two layers of alpha 0.35 and white over black: the first stores 0.35 * 255 = 89.25 -> 89; the second 0.35 + (89 / 255) 0.65 = 0.57686 -> 147.1 -> 147; kept in
    float it is 0.35 + 0.35 * 0.65 = 0.5775 -> 147.26.  Over a destination of 200: 0.35 + 0.65 * 200 / 255 = 0.8598 -> 219.25 -> 219."""
    full = [(-1.0, 1.0, 0.5, 1.0), (3.0, 1.0, 0.5, 1.0), (-1.0, -3.0, 0.5, 1.0)]
    col = [(1.0, 1.0, 1.0, 0.35)] * 3
    r = _draw([_instance(full + full, col + col)])
    assert (r["lo"][1, 1] == 147).all() and (r["hi"][1, 1] == 147).all() and r["layers"][1, 1] == 2
    t = np.full((4, 4, 4), 200, dtype=np.uint8)
    r = _draw([_instance(full, col)], target=t)
    assert (r["lo"][2, 2] == 219).all() and (r["hi"][2, 2] == 219).all()
    r = _draw([_instance(full, col, scissor=(1, 0, 2, 1))], target=t)        # the bottom row's two middle pixels only
    assert np.array_equal(r["layers"], np.array([[0] * 4] * 3 + [[0, 1, 1, 0]])) and (r["lo"][0, 0] == 200).all()
    r = _draw([_instance(full, col)], target=t, rows=np.array([False, True, False, False]))
    assert np.array_equal(r["layers"].any(axis=1), [False, True, False, False])


# ---- the oracle, case by case --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RC.CASES)
def test_oracle_rasteriser_within_the_rule(sample_data, oracle_lib, name):
    case, images, rule = _oracle(sample_data, oracle_lib, name)
    RC.hold(case, images, "oracle", rule=rule)


@pytest.mark.parametrize("name", ["layers", "textured"])
def test_oracle_foreground_list_over_a_ray_traced_frame_within_the_rule(sample_data, oracle_lib, name):
    """The sample's sphere and floor stay: the foreground list lies over the UNORM8 of the ray-traced OUTPUT, the background list goes to gBackground only."""
    case = RC.make_case(sample_data, name, over_ray_traced=True)
    images = RC.oracle_images(case)
    assert (RC.base_bytes(images["output"])[..., :3] > 0).mean() > 0.5
    RC.hold(case, images, "oracle/over-rt")


def test_oracle_one_instance_per_triangle_is_the_same_picture(sample_data, oracle_lib):
    """Instances in scene order, triangles in index order: a list split into one instance per triangle draws the same bytes."""
    case, images, rule = _oracle(sample_data, oracle_lib, "winding")
    split = RC.make_case(sample_data, "winding", split=True)
    assert len(split["data"].instances) > 16
    got = RC.oracle_images(split)
    assert np.array_equal(got["final"], images["final"])
    RC.hold(split, got, "oracle/split", rule=rule)


def test_the_case_tables_are_complete():
    assert set(RC.MUTATION_CASE) == set(R.MUTATIONS) and set(RC.MUTATION_CASE.values()) <= set(RC.CASES) and set(RC.SHARES) == set(RC.CASES)
    assert set(RC.EXACT) <= set(RC.CASES)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put the oracle outside the rule on a decided pixel of the case built to catch it (raster_cases.MUTATION_CASE); the right rule has none."""
    name = RC.MUTATION_CASE[mutation]
    case, images, rule = _oracle(sample_data, oracle_lib, name)
    wrong = RC.run_rule(case, mutate=mutation)
    bad = bad_right = und = 0
    for key in ("final", "background"):
        if rule[key] is None:
            continue
        bad_right += R.judge(rule[key], images[key])["wrong"]
        j = R.judge(wrong[key], images[key])
        bad += j["wrong"]; und += j["undecided"]
    print("raster_rule mutation %-40s case %-13s bad=%d undecided=%d" % (mutation, name, bad, und))
    assert bad_right == 0
    assert bad > 0 and und <= int(RC.UNDECIDED_CAP * RC.W * RC.H) * 2, "the case built for %s, %s, does not tell it from the rule" % (mutation, name)
