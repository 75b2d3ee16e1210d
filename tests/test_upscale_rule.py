"""tests/upscale_rule.py pinned on the CPU: a hand-made 5 x 4 -> 8 x 6 example whose numbers are written out, the Halton and quality-table restatements against the
oracle, the oracle's upscaler (`oupscale_frame`) held to the rule pixel by pixel in every case of tests/upscale_cases.py it can draw, and the named wrong variants of the
rule, each of which must put the oracle outside the rule in the case built to catch it.

The asserted conditions are the rule's: every channel of UPSCALED within value +- bound (ratio < 1), the count channel within its bound and exact where
the rule says so, no pixel undecided or uncovered.  MIN_BAD states for each variant at least how many pixels (summed over the case's compared frames) leave it: half of
what the oracle shows (profiles/upscale_rule_deviation.txt).  `tie_takes_last` has no frame: pixels of equal depth under a moving camera have equal flow, so it is
shown on a hand-made image that the oracle's own function upscales."""
import ctypes as C
import math

import numpy as np
import pytest

import upscale_cases as UC
import upscale_rule as UR

_sessions = {}
MIN_BAD = {"jitter_subtracted": 7614, "floor_without_jitter": 2011, "distance_from_clamped_index": 553, "sigma_two": 7584, "flow_of_centre": 1544, "flow_of_farthest": 1594,
           "flow_in_display_pixels": 4662, "flow_subtracted": 5044, "masks_of_nearest_depth": 2074, "history_nearest": 4473, "history_no_half_texel": 7172,
           "off_screen_clamped_not_dropped": 98, "no_colour_clamp": 402, "lock_ignored": 269, "lock_inverted": 410, "reactive_ignored": 2360, "conf_dropped": 939,
           "one_over_n": 5435, "cap_64": 627, "history_is_sharpened": 7187}


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = UC.make_case(sample_data, name)
        _sessions[name] = (case, UC.oracle_session(case))
    return _sessions[name]


# ---- the restatements -----------------------------------------------------------------------------------------------------------------------------------

def test_quality_table_restatement_is_the_oracles(oracle_lib):
    for up in (UR.UPSCALER_AUTO, UR.UPSCALER_FSR):
        for mode in range(7):
            for dw, dh in ((81, 47), (65, 41), (64, 40), (33, 19), (320, 180), (1280, 720), (1920, 1080), (2560, 1440), (3840, 2160), (7680, 4320), (1, 1), (2, 3)):
                a, b, c = C.c_int(), C.c_int(), C.c_int()
                assert oracle_lib.oracle_upscaler_info(up, mode, dw, dh, a, b, c) == 1
                assert UR.quality(mode, dw, dh) == (a.value, b.value, c.value), (mode, dw, dh)
    assert UR.quality(UR.MODE_QUALITY, 81, 47) == (54, 31, 18) and [UR.quality(UC.MODE_NAMES[n], 81, 47)[:2] for n in UC.RENDER] == list(UC.RENDER.values())


def test_jitter_restatement_is_the_oracles(sample_data, oracle_lib):
    """The oracle's pixelJitter of 40 frames in the quality mode (18 phases: two whole periods and a part) and of 10 in the native one (8 phases)."""
    from oracle import oracle_py
    for mode, frames in ((UR.MODE_QUALITY, 40), (UR.MODE_NATIVE, 10)):
        o = oracle_py.OracleScene(sample_data)
        try:
            phases = UR.quality(mode, 33, 19)[2]
            for f in range(frames):
                r = o.render(33, 19, upscaler=UR.UPSCALER_FSR, upscalerMode=mode)
                assert tuple(np.float32(r["pixelJitter"])) == tuple(np.float32(UR.jitter(f, phases))), (mode, f)
        finally:
            o.close()
    assert UR.jitter(0, 18) == (0.0, float(np.float32(1.0) / np.float32(3.0) - np.float32(0.5))) and UR.jitter(18, 18) == UR.jitter(0, 18)


# ---- the hand-made example ------------------------------------------------------------------------------------------------------------------------------

RW, RH, DW, DH = 5, 4, 8, 6
JITTER = (0.25, -0.25)


def _inputs(lock=0.0, reactive=0.0, flow=(0.3125, 0.0)):
    """Render image: red (8 i + k) / 64, green (8 k + i) / 64, blue (i + 5 k + 1) / 64.  Depth 10 + i + 4 k: the nearest of any window is its first tap.
    Previous image: red 0.5, green (x + 8 y) / 64, blue 0, count 3."""
    i, k = np.meshgrid(np.arange(RW), np.arange(RH), indexing="xy")
    color = np.stack([(8 * i + k) / 64.0, (8 * k + i) / 64.0, (i + 5 * k + 1) / 64.0, np.ones((RH, RW))], axis=-1).astype(np.float32)
    fl = np.broadcast_to(np.array(flow, dtype=np.float32), (RH, RW, 2)).copy()
    x, y = np.meshgrid(np.arange(DW), np.arange(DH), indexing="xy")
    prev = np.stack([np.full((DH, DW), 0.5), (x + 8 * y) / 64.0, np.zeros((DH, DW)), np.full((DH, DW), 3.0)], axis=-1).astype(np.float32)
    return dict(color=color, flow=fl, reactive=np.full((RH, RW), reactive, dtype=np.float32), lock=np.full((RH, RW), lock, dtype=np.float32),
                depth=(10.0 + i + 4 * k).astype(np.float32), prev=prev)


def _rule(i, prev=True, mutate=None):
    return UR.upsample(i["color"], i["flow"], i["reactive"], i["lock"], i["depth"], JITTER, i["prev"] if prev else None, (DW, DH), mutate=mutate)


def _oracle_upscale(oracle_lib, i, prev=True):
    fp = C.POINTER(C.c_float)
    arrays = [np.ascontiguousarray(i[k], dtype=np.float32) for k in ("color", "flow", "reactive", "lock", "depth", "prev")]
    out = np.zeros((DH, DW, 4), dtype=np.float32)
    f = oracle_lib.oupscale_frame
    f.restype = None
    f.argtypes = [fp] * 5 + [C.c_int, C.c_int, C.c_float, C.c_float, fp, fp, C.c_int, C.c_int, C.c_int]
    f(*[a.ctypes.data_as(fp) for a in arrays[:5]], RW, RH, JITTER[0], JITTER[1], arrays[5].ctypes.data_as(fp), out.ctypes.data_as(fp), DW, DH, int(prev))
    return out


# Display pixel (3, 2): u = 3.5 / 8, r.x = 2.1875; v = 2.5 / 6, r.y = 5 / 3.  r - j = (1.9375, 1.9167): (i0, k0) = (1, 1), the window is columns 0..2, rows 0..2.
# Samples at i + 0.75 and k + 0.25: the distances below.  w = exp(-2 d^2), separable.
DX, DY = (1.4375, 0.4375, -0.5625), (17.0 / 12.0, 5.0 / 12.0, -7.0 / 12.0)


def _weights():
    return [[math.exp(-2.0 * (dx * dx + dy * dy)) for dx in DX] for dy in DY]                   # [k][i]


def _mean(channel):
    w = _weights()
    total = sum(w[k][i] for k in range(3) for i in range(3))
    return sum(w[k][i] * channel(i, k) for k in range(3) for i in range(3)) / total


CUR = (lambda: (_mean(lambda i, k: (8 * i + k) / 64.0), _mean(lambda i, k: (8 * k + i) / 64.0), _mean(lambda i, k: (i + 5 * k + 1) / 64.0)))


def test_hand_made_example_without_a_history(oracle_lib):
    i = _inputs()
    r = _rule(i, prev=False)
    assert np.abs(r["value"][2, 3] - np.array(CUR())).max() < 1e-9          # (the kernel's constant 2.88539008f is 2 / ln 2 to float32 precision: the weights agree to 1e-7)
    c = r["info"]["counts"]
    assert c["fresh"] == DW * DH and (r["count"] == 1.0).all() and r["count_exact"].all() and c["not_decided"] == 0 and c["not_covered"] == 0
    # the nearest depth of every window is its first tap, which is the centre only where the window is clamped on both axes: (i0, k0) = (0, 0)
    assert c["flow_not_centre"] == DW * DH - int((r["masks"]["taps_clamped_left"] & r["masks"]["taps_clamped_top"]).sum()) and c["depth_tie"] == 0
    # r.x - 0.25 of the eight columns: 0.0625, 0.6875, 1.3125, 1.9375, 2.5625, 3.1875, 3.8125, 4.4375: i0 = 0 0 1 1 2 3 3 4, none clamped
    assert (c["taps_clamped_left"], c["taps_clamped_right"], c["i0_clamped"]) == (2 * DH, 1 * DH, 0)
    # r.y + 0.25 of the six rows: 0.5833, 1.25, 1.9167, 2.5833, 3.25, 3.9167: k0 = 0 1 1 2 3 3
    assert (c["taps_clamped_top"], c["taps_clamped_bottom"], c["k0_clamped"]) == (1 * DW, 2 * DW, 0)
    up = _oracle_upscale(oracle_lib, i, prev=False)
    cmp = UR.compare(up, r)
    assert not cmp["bad"].any() and not cmp["count_bad"].any() and cmp["largest"] < 1.0


def test_hand_made_example_with_a_history(oracle_lib):
    """flow (0.3125, 0) of 5 render pixels is 0.0625 in u: uvPrev = (0.5, 2.5 / 6), the history position (3.5, 2): half of display pixels (3, 2) and (4, 2).
    History: red 0.5, green 19.5 / 64, blue 0, N = 3.  The box of the window: red and green 0 .. 18 / 64, blue 1 / 64 .. 13 / 64: all three channels are clamped."""
    cur = np.array(CUR())
    hist = np.array([0.5, 19.5 / 64.0, 0.0])
    box = np.array([18.0 / 64.0, 18.0 / 64.0, 1.0 / 64.0])
    conf = _weights()[1][1]
    assert 0.1 * conf < 0.25                                                        # 1 / (N + 1) = 1 / 4 sets the blend factor
    for lock, reactive, a in ((0.0, 0.0, 0.25), (128.0 / 255.0, 0.0, 0.25), (0.0, 204.0 / 255.0, 204.0 / 255.0), (1.0, 51.0 / 255.0, 0.25)):
        i = _inputs(lock=lock, reactive=reactive)
        r = _rule(i)
        lk, re = float(np.float32(lock)), float(np.float32(reactive))
        hc = box + lk * (hist - box)
        want = hc + max(a, re) * (cur - hc)
        assert np.abs(r["value"][2, 3] - want).max() < 1e-7, (lock, reactive, r["value"][2, 3], want)
        assert abs(r["count"][2, 3] - 4.0) < 1e-6 and r["masks"]["outside_box"][2, 3] and r["masks"]["locked_outside_box"][2, 3] == (lock > 0)
        assert r["masks"]["reactive_wins"][2, 3] == (reactive > 0.25) and r["masks"]["count_wins"][2, 3] == (reactive < 0.25)
        up = _oracle_upscale(oracle_lib, i)
        cmp = UR.compare(up, r)
        assert not cmp["bad"].any() and not cmp["count_bad"].any() and cmp["largest"] < 1.0, (lock, reactive, cmp["largest"])
    # a flow that leaves the screen: 3 render pixels to the right are 0.6 in u; columns 4..7 (u > 0.4) have no history and start over
    r = _rule(_inputs(flow=(3.0, 0.0)))
    assert r["masks"]["history_off_screen"][:, 4:].all() and not r["masks"]["history_off_screen"][:, :3].any() and (r["count"][:, 4:] == 1.0).all()
    # the cap: a history of 32 stays 32, one of 31 becomes 32, and the rule says where that is exact
    i = _inputs(flow=(0.0, 0.0)); i["prev"][..., 3] = 32.0
    r = _rule(i)
    assert (r["count"] == 32.0).all() and r["count_exact"].all() and r["info"]["counts"]["capped"] == DW * DH
    assert (_rule(i, mutate="cap_64")["count"] == 33.0).all()


def test_the_first_of_equal_depths_gives_the_flow(oracle_lib):
    """`tie_takes_last`: every depth equal, every column its own flow, the lock mask 1 so that the history the flow fetches reaches the output."""
    i = _inputs(lock=1.0)
    i["depth"][:] = 1.0
    i["flow"][..., 0] = 0.0625 * np.arange(RW)[None, :]
    i["color"][..., :3] = 0.25
    r = _rule(i)
    assert r["info"]["counts"]["depth_tie"] == DW * DH
    up = _oracle_upscale(oracle_lib, i)
    cmp = UR.compare(up, r)
    assert not cmp["bad"].any() and cmp["largest"] < 1.0
    wrong = UR.compare(up, _rule(i, mutate="tie_takes_last"))
    print("upscale_rule oracle %-32s %-17s bad=%d" % ("tie_takes_last", "hand-made", int(wrong["bad"].sum())))
    assert int(wrong["bad"].sum()) >= DW * DH // 2


def test_a_value_that_is_not_finite_is_not_covered():
    i = _inputs(); i["color"][1, 2, 1] = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        r = _rule(i)
    stored = np.concatenate([r["value"], r["count"][..., None]], axis=-1)
    with np.errstate(invalid="ignore"):
        assert r["info"]["counts"]["not_covered"] > 0 and int(UR.compare(stored, r)["bad"].sum()) == r["info"]["counts"]["not_covered"]
    assert _rule(_inputs())["info"]["counts"]["not_covered"] == 0


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", UC.CASES)
def test_oracle_upscaled_within_the_rule(sample_data, oracle_lib, name):
    case, frames = _oracle(sample_data, oracle_lib, name)
    UC.hold(case, frames, "oracle")


@pytest.mark.parametrize("mutation", [m for m in UR.MUTATIONS if m not in UC.HAND_MADE])
def test_wrong_variant_puts_the_oracle_outside_the_rule(sample_data, oracle_lib, mutation):
    name = UC.MUTATION_CASE[mutation]
    case, frames = _oracle(sample_data, oracle_lib, name)
    bad = []
    for n in case["compared"]:
        c = UR.compare(frames[n]["upscaled"], UC.run_rule(case, frames, n, mutate=mutation))
        bad.append(int((c["bad"] | c["count_bad"]).sum()))
    print("upscale_rule oracle %-32s %-17s bad=%s" % (mutation, name, bad))
    assert sum(bad) >= MIN_BAD[mutation], (mutation, bad)


def test_every_variant_has_a_case():
    assert set(UR.MUTATIONS) == set(UC.MUTATION_CASE) | set(UC.HAND_MADE) and set(MIN_BAD) == set(UC.MUTATION_CASE)
