"""tests/compose_rule.py pinned on the CPU: hand-made 4 x 3 and 5 x 2 images whose every texel has its own value, the oracle's ComposePS (`pass_compose_post`) held to
the rule pixel by pixel in every compose case of tests/post_cases.py, and the named wrong variants of the rule, each of which must put the oracle outside the rule in
the case built to catch it.

The bound is the rule's: the asserted ratio is < 1, no pixel is left uncovered, the back buffer lies in the UNORM8 interval of value +- bound and is
the conversion of the stored float32 byte for byte.  MIN_BAD states for each variant at least how many pixels leave it: half of what the oracle shows
(profiles/compose_post_rule_deviation.txt)."""
import numpy as np
import pytest

import compose_rule as CR
import post_cases as PCS

_sessions = {}
AMBIENT = ((0.1, 0.1, 0.1), (0.2, 0.2, 0.2))
MIN_BAD = {"no_alpha_lerp": 72, "reflection_dropped": 384, "indirect_not_f16_on_lean": 500, "lean_reads_filtered": 500}


def _oracle(sample_data, oracle_lib, name):
    if name not in _sessions:
        case = PCS.make_case(sample_data, name)
        _sessions[name] = (case, PCS.oracle_session(case))
    return _sessions[name]


# ---- hand-made images ---------------------------------------------------------------------------------------------------------------------------------

def _images(w=4, h=3, alpha=None):
    """Every texel its own value: diffuse bytes 10 + 7 x + 29 y (+ 3 per channel), alpha 255 unless given (a byte, or an (h, w) array of bytes); the light and the
    additive images in sixteenths, all float16 values."""
    x, y = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    k = np.stack([10 + 7 * x + 29 * y + 3 * c for c in range(3)] + [np.broadcast_to(255 if alpha is None else alpha, (h, w))], axis=-1)
    f16 = lambda a: np.concatenate([a, np.ones((h, w, 1))], axis=-1).astype(np.float16).astype(np.float32)
    grid = lambda base, sx, sy: f16(np.stack([base + (sx * x + sy * y + c) / 16.0 for c in range(3)], axis=-1))
    return dict(diffuse=(k / 255.0).astype(np.float32), direct=grid(0.25, 1, 2), indirect=grid(0.0625, 2, 1), direct_raw=grid(0.5, 1, 1),
                reflection=grid(0.0, 1, 0), refraction=grid(0.0, 0, 1), transparent=grid(0.125, 1, 1))


def _by_hand(img, lean=False):
    """The sentence of ComposePS, written out once more in plain float64."""
    d = img["diffuse"].astype(np.float64)
    a = d[..., 3:4]
    if lean:
        amb = (np.float32(0.1) + np.float32(0.2)).astype(np.float16).astype(np.float64)
        lit = d[..., :3] + a * (d[..., :3] * (img["direct_raw"][..., :3].astype(np.float64) + amb) - d[..., :3])
    else:
        lit = d[..., :3] + a * (d[..., :3] * (img["direct"][..., :3].astype(np.float64) + img["indirect"][..., :3]) - d[..., :3])
        lit = lit + img["reflection"][..., :3] + img["refraction"][..., :3] + img["transparent"][..., :3]
    return np.where(a > 1e-6, lit, d[..., :3])


@pytest.mark.parametrize("size", [(4, 3), (5, 2)])
def test_the_lit_sentence_and_its_bound(size):
    img = _images(*size, alpha=153)
    r = CR.compose(img)
    assert r["lit"].all() and r["unorm8_inputs"].all() and r["covered"].all()
    assert np.abs(r["value"][..., :3] - _by_hand(img)).max() < 1e-15 and (r["value"][..., 3] == 1.0).all() and (r["bound"][..., 3] == 0.0).all()
    # seven operations of half an ulp each on values of a few units: the bound is a few 2^-24 of the largest operand, and never 0 on a lit pixel
    assert (r["bound"][..., :3] > 0).all() and (r["bound"][..., :3] < 16 * 2.0 ** -24 * 4.0).all()
    # a float32 evaluation, one rounding per operation, lies inside it
    f = np.float32
    d = img["diffuse"]
    res = d[..., :3] * (img["direct"][..., :3] + img["indirect"][..., :3])
    res = d[..., :3] + d[..., 3:4] * (res - d[..., :3])
    res = ((res + img["reflection"][..., :3]) + img["refraction"][..., :3]) + img["transparent"][..., :3]
    assert res.dtype == f and (CR.ratio(res, r["value"][..., :3], r["bound"][..., :3]) < 1.0).all()


def test_the_alpha_test_is_exact_and_the_unlit_pixel_is_the_diffuse_colour():
    alpha = np.array([[0, 1, 2, 255], [0, 128, 0, 254], [1, 0, 255, 0]])
    img = _images(alpha=alpha)
    r = CR.compose(img)
    assert np.array_equal(r["lit"], alpha > 0)                                    # 1 / 255 is far above 1e-6: nothing is undecided
    assert (r["value"][~r["lit"]][:, :3] == img["diffuse"][~r["lit"]][:, :3].astype(np.float64)).all() and (r["bound"][~r["lit"]] == 0.0).all()
    assert np.abs(r["value"][..., :3] - _by_hand(img)).max() < 1e-15
    c = r["info"]["counts"]
    assert (c["lit"], c["unlit"], c["partial"], c["opaque"]) == (7, 5, 5, 2)
    # the variant that takes the branch at a = 0 too adds the three images there: only a hand-made image has any (post_cases.COMPOSE_MUTATION_CASE says why)
    wrong = CR.compose(img, mutate="alpha_test_ge")
    bad = ~(CR.ratio(r["value"], wrong["value"], wrong["bound"]).max(axis=-1) < 1.0)
    print("compose_rule hand-made alpha_test_ge bad=%d" % bad.sum())
    assert np.array_equal(bad, alpha == 0)
    extra = (img["reflection"] + img["refraction"] + img["transparent"])[..., :3].astype(np.float64)
    assert np.abs(wrong["value"][alpha == 0][:, :3] - (img["diffuse"][..., :3].astype(np.float64) + extra)[alpha == 0]).max() < 1e-6


def test_wrong_variants_differ_on_hand_made_images():
    img = _images(alpha=153)
    r = CR.compose(img)
    for m in ("no_alpha_lerp", "reflection_dropped"):
        w = CR.compose(img, mutate=m)
        bad = ~(CR.ratio(r["value"], w["value"], w["bound"]).max(axis=-1) < 1.0)
        assert bad.sum() >= 9, (m, bad.sum())                                       # (reflection is 0 in the first column of the red channel only)
    assert (CR.compose(_images(alpha=255), mutate="no_alpha_lerp")["value"] == CR.compose(_images(alpha=255))["value"]).all()      # lerp(d, x, 1) = x: alpha 1 cannot show it


def test_a_lean_frame_reads_the_raw_direct_light_and_the_constant_ambient():
    img = _images(5, 2)
    r = CR.compose(img, lean=True, ambient=AMBIENT)
    assert np.abs(r["value"][..., :3] - _by_hand(img, lean=True)).max() < 1e-15
    # 0.1f + 0.2f = 0.3 (+ 1.2e-8) is not a float16: the image holds 0.300048828125
    assert (CR.ambient_constant(*AMBIENT) == 0.300048828125).all() and abs(CR.ambient_constant(*AMBIENT, mutate="indirect_not_f16_on_lean")[0] - 0.3) < 1e-7
    for m in ("indirect_not_f16_on_lean", "lean_reads_filtered"):
        w = CR.compose(img, lean=True, ambient=AMBIENT, mutate=m)
        assert not (CR.ratio(r["value"], w["value"], w["bound"]).max(axis=-1) < 1.0).any(), m
    only = {k: img[k] for k in ("diffuse", "direct_raw")}                              # it reads nothing else
    assert (CR.compose(only, lean=True, ambient=AMBIENT)["value"] == r["value"]).all()


def test_unorm8_conversion_and_its_interval():
    assert list(CR.unorm8([-1.0, 0.0, 0.5 / 255.0, 0.49 / 255.0, 1.0, 2.0, 127.5 / 255.0])) == [0, 0, 1, 0, 255, 255, 128]
    assert list(CR.unorm8_of_float32(np.array([np.nan, -0.0, 1e-9, 0.999, 1.5, np.inf], dtype=np.float32))) == [0, 0, 0, 255, 255, 255]
    lo, hi = CR.to_final(np.array([0.3, 100.5 / 255.0, 1.2]), np.array([1e-7, 1e-7, 1e-7]))
    assert list(lo) == [76, 100, 255] and list(hi) == [77, 101, 255]               # 0.3 x 255 = 76.5 is a tie of the conversion, like 100.5: both bytes are held
    lo, hi = CR.to_final(np.array([0.3]), np.array([0.0]))
    assert (lo[0], hi[0]) == (76, 77)                                               # even an exact 0.3 is 76.49999... or 76.50000... after 255 x in float32
    bad = _images(); bad["diffuse"][1, 2, 0] += np.float32(1e-4)
    r = CR.compose(bad)
    assert r["info"]["counts"]["not_unorm8"] == 1 and not r["unorm8_inputs"][1, 2]


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PCS.COMPOSE_CASES)
def test_oracle_compose_within_the_rule(sample_data, oracle_lib, name):
    case, img = _oracle(sample_data, oracle_lib, name)
    PCS.hold_compose(case, img, "oracle")
    if case["lean"]:
        # the oracle writes every image of every frame: the same frame is held by the sentence of a full frame too
        full = dict(case, lean=False, name=name)
        PCS.hold_compose(full, img, "oracle/as-full")


def test_oracle_primary_spp_back_buffer_is_the_conversion_of_its_output(sample_data, oracle_lib):
    case, img = _oracle(sample_data, oracle_lib, "spp")
    assert (img["final"] == CR.unorm8_of_float32(img["output"])).all()


@pytest.mark.parametrize("mutation", sorted(PCS.COMPOSE_MUTATION_CASE))
def test_wrong_variant_puts_the_oracle_outside_the_rule(sample_data, oracle_lib, mutation):
    name = PCS.COMPOSE_MUTATION_CASE[mutation]
    case, img = _oracle(sample_data, oracle_lib, name)
    if mutation == "lean_reads_filtered":
        # a lean frame does not write the filtered images: a kernel that read them would find what the last full frame left.  Here that is a frame of the same scene
        # with one GI sample, drawn by a session of its own
        stale = PCS.oracle_session(case, giSamples=1)
        img = dict(img, direct=stale["direct"], indirect=stale["indirect"])
    r = PCS.run_compose(case, img, mutate=mutation)
    c = CR.compare(img["output"], img["final"], r)
    print("compose_rule oracle %-26s %-8s bad=%d final_bad=%d" % (mutation, name, int(c["bad"].sum()), c["final_bad"]))
    assert int(c["bad"].sum()) >= MIN_BAD[mutation], (mutation, int(c["bad"].sum()))
    assert set(PCS.COMPOSE_MUTATION_CASE) | {"alpha_test_ge"} == set(CR.MUTATIONS)
