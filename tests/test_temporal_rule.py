"""tests/temporal_rule.py pinned on the CPU: hand-made 4 x 3 frames, the oracle's temporal accumulation (`history_weight` / `pass_indirect`) held to the rule pixel
by pixel in every case of tests/temporal_cases.py with its twin session, and the named wrong variants of the rule, each of which must put the oracle outside the
rule in the case built to catch it.

The bound is the rule's: the asserted ratio is < 1 for rgb, alpha and both moments; at most 0.1 % of a frame's surface pixels may be undecided
(temporal_cases.UNDECIDED_CAP) and none uncovered but in `cap`."""
import numpy as np
import pytest

import temporal_cases as TC
import temporal_rule as T

_sessions, _rules = {}, {}
AMBIENT = ((0.125, 0.125, 0.125), (0.25, 0.25, 0.25))


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = TC.make_case(sample_data, name)
        _sessions[name] = (case, TC.oracle_session(case))
        _rules[name] = {}
    return _sessions[name]


# ---- hand-made frames -------------------------------------------------------------------------------------------------------------------------------

def _frame(flow=(0.0, 0.0), history=4.0, normal=(0.0, 0.0, 1.0), prev_normal=(0.0, 0.0, 1.0), depth=0.5, prev_depth=0.5):
    """4 x 3: every previous pixel holds its own colour (x + 1) / 8, (y + 1) / 4, 0.5 and moments (x + 1) / 16, (y + 1) / 32; the fresh sample is (1, 0.5, 0.25),
    moments (0.75, 0.625)."""
    h, w = 3, 4
    x, y = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    full = lambda v, c: np.broadcast_to(np.asarray(v, dtype=np.float32), (h, w, c)).copy()
    cur = dict(flow=full(flow, 2), depth=np.full((h, w), depth, dtype=np.float32), normal=full(tuple(normal) + (0.0,), 4), id=np.zeros((h, w), dtype=np.int32))
    raw = np.stack([(x + 1) / 8.0, (y + 1) / 4.0, np.full(x.shape, 0.5), np.full(x.shape, history)], axis=-1).astype(np.float32)
    prev = dict(raw=raw, moments=np.stack([(x + 1) / 16.0, (y + 1) / 32.0], axis=-1).astype(np.float32), depth=np.full((h, w), prev_depth, dtype=np.float32),
                normal=full(tuple(prev_normal) + (0.0,), 4))
    fresh = dict(raw=full((1.0, 0.5, 0.25, 1.0), 4), moments=full((0.75, 0.625), 2))
    return cur, prev, fresh


def _run(frame, samples=1, **kw):
    return T.accumulate(frame[0], frame[1], frame[2], samples, AMBIENT, **kw)


def test_the_cast_truncates_toward_zero():
    """x + 0.5 + flow.x = -0.5 at column 0 lands ON column 0 (N1); with floor it is column -1, no history.  -1.0 is off the frame either way.  The same in y."""
    for axis in (0, 1):
        flow = [0.0, 0.0]; flow[axis] = -1.0
        r = _run(_frame(flow=flow))
        edge = (slice(None), 0) if axis == 0 else (0, slice(None))
        assert r["decided"].all() and r["inside"][edge].all() and (r["prev_x" if axis == 0 else "prev_y"][edge] == 0).all()
        assert np.allclose(r["value"][edge][:, 3], 5.0) and not r["zero_history"].any()
        assert r["info"]["counts"]["truncation_x" if axis == 0 else "truncation_y"] == (3 if axis == 0 else 4)
        wrong = _run(_frame(flow=flow), mutate="floor_not_trunc")
        assert not wrong["inside"][edge].any() and (wrong["value"][edge][:, 3] == 1.0).all()
        flow[axis] = -1.5
        assert not _run(_frame(flow=flow))["inside"][edge].any()
    # the half pixel: a flow of +0.5 reaches the next pixel, one of +0.4375 does not
    assert (_run(_frame(flow=(0.5, 0.0)))["prev_x"][:, :3] == [1, 2, 3]).all() and (_run(_frame(flow=(0.4375, 0.0)))["prev_x"] == [0, 1, 2, 3]).all()
    assert (_run(_frame(flow=(0.5, 0.0)), mutate="no_half_pixel")["prev_x"] == [0, 1, 2, 3]).all()
    assert (_run(_frame(flow=(1.0, 0.0)), mutate="flow_subtracted")["prev_x"][:, 1:] == [0, 1, 2]).all()
    # a flow the float32 sum cannot carry is refused, not guessed
    assert not _run(_frame(flow=(4096.0, 0.0)))["decided"].any()


def test_loads_off_the_frame_are_zero_on_all_four_sides():
    """A previous pixel off any edge: depth, normal, colour, history and moments are 0, so h0 = 0 exactly, h = 1, the stored colour is the fresh float16 within its
    half step, alpha 1 and the moments the fresh ones."""
    for flow, gone in (((-2.5, 0.0), (slice(None), slice(0, 2))), ((1.5, 0.0), (slice(None), slice(2, 4))), ((0.0, -2.5), (slice(0, 2), slice(None))),
                       ((0.0, 1.5), (slice(1, 3), slice(None)))):
        r = _run(_frame(flow=flow))
        assert not r["inside"][gone].any() and r["zero_history"][gone].all() and r["inside"].sum() == 12 - r["zero_history"].sum()
        assert (r["value"][gone] == [1.0, 0.5, 0.25, 1.0]).all() and (r["bound"][gone][..., 3] == 0).all() and (r["moments"][gone] == [0.75, 0.625]).all()
        assert (r["bound"][gone][..., :3] < 1.001 * 2.0 ** -10 * np.array([1.0, 0.5, 0.25])).all() and (r["moments_bound"][gone] < 1e-6).all() and (r["bound"][~r["zero_history"]][..., 3] > 0).all()
        clamped = _run(_frame(flow=flow), mutate="edge_clamped_not_zero")
        assert (clamped["value"][gone][..., 3] == 5.0).all()


def test_pow_of_zero_is_zero_and_the_depth_term():
    r = _run(_frame(prev_normal=(1.0, 0.0, 0.0)))
    assert r["zero_history"].all() and (r["weight"].v == 0).all() and (r["weight"].e == 0).all() and (r["value"][..., 3] == 1.0).all()
    r = _run(_frame(prev_normal=(0.0, 0.0, -1.0)))                                  # max(0, -1)
    assert r["zero_history"].all()
    r = _run(_frame(depth=0.5, prev_depth=0.51))                                    # exp(-1) within float32's roundings of 0.51 - 0.5 and of 0.01f
    assert np.allclose(r["weight"].v, np.exp(-1.0), rtol=1e-5) and np.allclose(r["value"][..., 3], 4.0 * np.exp(-1.0) + 1.0, rtol=1e-5) and (r["weight"].e < 2e-5).all()
    assert np.allclose(_run(_frame(depth=0.5, prev_depth=0.51), mutate="depth_scale_tenth")["weight"].v, np.exp(-0.1), rtol=1e-5)
    r = _run(_frame(depth=0.0, prev_depth=1.5))                                     # exp(-150) is 0 in float32
    assert r["zero_history"].all()


def test_a_weight_above_one_grows_the_history_by_more_than_one():
    """Float16 normals of length 1 + 2^-10: the cosine is (1 + 2^-10)^2 and the weight its 128th power, 1.284: a history of 10 becomes 13.84, not 11."""
    n = (0.0, 0.0, 1.0 + 2.0 ** -10)
    r = _run(_frame(history=10.0, normal=n, prev_normal=n))
    w = (1.0 + 2.0 ** -10) ** 256
    assert np.allclose(r["weight"].v, w, rtol=1e-12) and np.allclose(r["value"][..., 3], 10.0 * w + 1.0) and (r["value"][..., 3] > 13.8).all()
    assert r["info"]["counts"]["above_one"] == 12 and r["info"]["counts"]["grown"] == 12
    assert (r["weight"].e / w < 2e-4).all() and (r["bound"][..., 3] < 2.0 ** -8 + 3e-3).all()
    assert np.allclose(_run(_frame(history=10.0, normal=n, prev_normal=n), mutate="weight_clamped_at_one")["value"][..., 3], 11.0)
    assert np.allclose(_run(_frame(history=10.0, normal=n, prev_normal=n), mutate="normal_exponent_64")["weight"].v, (1.0 + 2.0 ** -10) ** 128)
    half = (0.0, 0.0, 0.5)
    assert np.allclose(_run(_frame(history=10.0, normal=half, prev_normal=n), mutate="history_unweighted")["value"][..., 3], 11.0)


def test_the_cap():
    """64 stays 64, exactly; 63.40625 + 1 is capped to 64 (a cap taken before the increment gives 64.40625, no cap the same); the colour moves by 1 / 64 of the way."""
    r = _run(_frame(history=64.0))
    assert (r["value"][..., 3] == 64.0).all() and (r["bound"][..., 3] == 0.0).all() and r["info"]["counts"]["capped"] == 12 and r["info"]["counts"]["capped_before"] == 12
    r = _run(_frame(history=63.40625))
    assert (r["value"][..., 3] == 64.0).all() and (r["bound"][..., 3] == 0.0).all()
    prev = _frame()[1]["raw"].astype(np.float64)
    assert np.allclose(r["value"][..., :3], prev[..., :3] + (np.array([1.0, 0.5, 0.25]) - prev[..., :3]) / 64.0, rtol=0, atol=1e-12)
    assert np.allclose(r["moments"], _frame()[1]["moments"] + (np.array([0.75, 0.625]) - _frame()[1]["moments"]) / 64.0, rtol=0, atol=1e-12)
    for m in ("cap_before_increment", "no_cap"):
        assert np.allclose(_run(_frame(history=63.40625), mutate=m)["value"][..., 3], 64.40625)
    assert np.allclose(_run(_frame(history=64.0), mutate="cap_before_increment")["value"][..., 3], 65.0)
    # under the cap: h = 5, the colour a fifth of the way, within half a float16 step and the fresh sample's own fifth
    r = _run(_frame())
    assert np.allclose(r["value"][..., :3], prev[..., :3] + (np.array([1.0, 0.5, 0.25]) - prev[..., :3]) / 5.0, rtol=0, atol=1e-12) and (r["value"][..., 3] == 5.0).all()
    assert (r["bound"][..., :3] >= T.f16_half_step(r["value"][..., :3])).all() and (r["bound"][..., :3] < 2.0 * T.f16_half_step(r["value"][..., :3]) + 1e-6).all()


def test_several_samples_and_the_pixels_the_closed_form_does_not_cover():
    """(N5) Two samples on a history of 4: (prev * 4 + 2 * mean) / 6 -- the same as two steps of the loop on any two samples with that mean; alpha 6; the moments move
    by 2 / 6.  On a history of 63 the cap binds inside the loop: not covered."""
    f = _frame(); f[2]["raw"][..., 3] = 2.0
    r = _run(f, samples=2)
    prev = f[1]["raw"].astype(np.float64); mean = np.array([1.0, 0.5, 0.25])
    c = prev[..., :3]
    for k, s in enumerate((mean * 1.5, mean * 0.5)):
        c = c + (s - c) / (4.0 + k + 1.0)
    assert r["covered"].all() and np.allclose(r["value"][..., :3], c, rtol=0, atol=1e-12) and (r["value"][..., 3] == 6.0).all()
    assert np.allclose(r["moments"], f[1]["moments"] + (np.array([0.75, 0.625]) - f[1]["moments"]) * (2.0 / 6.0), rtol=0, atol=1e-12)
    assert not _run(_frame(history=63.0), samples=2)["covered"].any() and _run(_frame(history=61.0), samples=2)["covered"].all()
    assert np.allclose(_run(f, samples=2, mutate="moments_alpha_one")["moments"], [0.75, 0.625]) and (_run(f, samples=2, mutate="alpha_not_history")["value"][..., 3] == 2.0).all()


def test_the_moments_come_from_the_previous_pixel():
    r = _run(_frame(flow=(1.0, 0.0)))
    pm = _frame()[1]["moments"].astype(np.float64)
    assert np.allclose(r["moments"][:, :3], pm[:, 1:] + (np.array([0.75, 0.625]) - pm[:, 1:]) / 5.0, rtol=0, atol=1e-12) and (r["moments"][:, 3] == [0.75, 0.625]).all()
    assert (r["moments_bound"] < 1e-5).all() and (r["moments_bound"][:, :3] > 0).all()      # (the pow term of the weight, through h, is most of it)
    wrong = _run(_frame(flow=(1.0, 0.0)), mutate="moments_at_current_pixel")
    assert (np.abs(wrong["moments"][:, :3, 0] - r["moments"][:, :3, 0]) > 100 * r["moments_bound"][:, :3, 0]).all()
    here = _run(_frame(flow=(1.0, 0.0)), mutate="previous_at_current_pixel")
    assert (here["prev_x"] == [0, 1, 2, 3]).all() and here["inside"].all()
    # the guides are the PREVIOUS frame's: with the current frame's depth at j the difference vanishes
    assert np.allclose(_run(_frame(prev_depth=0.51), mutate="guides_of_current_frame")["weight"].v, 1.0)


def test_a_pixel_without_a_surface():
    f = _frame(); f[0]["id"][1, 2] = -1
    r = _run(f)
    assert (r["value"][1, 2] == [0.375, 0.375, 0.375, 0.0]).all() and (r["bound"][1, 2] == 0).all() and (r["moments"][1, 2] == 0).all() and (r["moments_bound"][1, 2] == 0).all()
    assert not r["surface"][1, 2] and r["surface"].sum() == 11 and r["decided"].all() and r["covered"].all()
    r = _run(_frame(), samples=0)
    assert not r["surface"].any() and (r["value"] == [0.375, 0.375, 0.375, 0.0]).all()
    # the sum is one float32 addition, the store one float16 rounding
    r = T.accumulate(f[0], f[1], f[2], 1, ((0.1, 0.1, 0.1), (0.2, 0.2, 0.2)))
    assert (r["value"][1, 2, :3] == float(np.float16(np.float32(0.1) + np.float32(0.2)))).all()


def test_compare_counts_only_decided_and_covered_pixels():
    f = _frame()
    r = _run(f)
    raw = r["value"].copy(); raw[0, 0, 3] += 0.5; raw[1, 1, 0] += 2.0 * r["bound"][1, 1, 0]
    ratios, bad = T.compare(raw, r["moments"], r)
    assert bad.sum() == 2 and bad[0, 0] and bad[1, 1] and ratios["alpha"][0] > 100.0 and 1.9 < ratios["rgb"][0] < 2.1 and ratios["moments"][0] == 0.0
    r["decided"][0, 0] = False; r["covered"][1, 1] = False
    assert T.compare(raw, r["moments"], r)[1].sum() == 0


# ---- the oracle, case by case -----------------------------------------------------------------------------------------------------------------------

def test_every_variant_has_its_case():
    assert set(TC.MUTATION_CASE) == set(T.MUTATIONS) and set(TC.SHARES) == set(TC.CASES)


@pytest.mark.parametrize("name", TC.CASES)
def test_oracle_accumulation_within_the_rule(sample_data, oracle_lib, name):
    case, sess = _oracle(sample_data, oracle_lib, name)
    TC.hold(case, sess, "oracle", rules=_rules[name])


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_every_wrong_variant_is_caught(sample_data, oracle_lib, mutation):
    """A wrong variant must put at least one decided pixel of the oracle outside it, in the case built to catch it (temporal_cases.MUTATION_CASE), and the right
    rule none."""
    name, n = TC.MUTATION_CASE[mutation]
    case, sess = _oracle(sample_data, oracle_lib, name)
    assert n in case["compared"]
    right = TC.judge(TC.run_rule(case, sess[n]), sess[n])
    wrong = TC.judge(TC.run_rule(case, sess[n], mutate=mutation), sess[n])
    print("temporal_rule mutation %-26s case %-13s frame %2d bad=%d undecided=%d/%d" % (mutation, name, n, wrong["bad"], wrong["undecided"], right["undecided"]))
    assert right["bad"] == 0
    assert wrong["bad"] >= 1, "the case built for %s, %s, does not tell it from the rule" % (mutation, name)
