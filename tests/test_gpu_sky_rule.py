"""The kernels' sky held to tests/sky_rule.py pixel by pixel (rules E1-E8), through the rule of the pass that shows it.

A case of tests/sky_cases.py is a session of the primary, GI or mirror cases with a sky DESCRIPTION in place of their one constant term: a generated texture, a
multiplier, an HSL modifier and a yaw offset.  The pass's rule is fed with the GPU's own stored inputs, as in tests/test_gpu_gi_rule.py and
tests/test_gpu_primary_rule.py, and every stored value must lie within the rule's bound at every pixel the rule decides (DIFFUSE: among the bytes the rule allows); at
most 0.5 % of the pixels that see the sky in the pass may be undecided.  The `record-` cases are run and written down, not gated.

The sky code is inlined into every kernel that shows it: each launch form that tests/test_gpu_gi_rule.py, tests/test_gpu_mirror_rule.py and
tests/test_gpu_primary_rule.py name runs on one case."""
import numpy as np
import pytest

import sky_cases as SC
from test_gpu_gi_rule import PATHS as GI_PATHS
from test_gpu_mirror_rule import PATHS as MIRROR_PATHS
from test_gpu_primary_rule import PATHS as PRIMARY_PATHS

pytestmark = pytest.mark.gpu

# launch form -> the case that runs on it (one each)
GI_FORMS = {"refill": "bounce", "split": "bounce-padded", "plain": "bounce-off", "no-lds-cache": "two-bounces", "general-kernels": "four-by-four",
            "four-workgroups": "bounce-two-by-two", "three-kernel-frame": "bounce-over-backdrop"}
MIRROR_FORMS = {"no-lds-cache": "mirror-floor", "general-kernels": "glass-sphere", "aux-stream": "mirror-floor"}
PRIMARY_FORMS = {"lean-frame": "level", "full-frame": "up", "gi-one-kernel": "seam", "gi-three-kernels": "sixteen-by-nine", "no-lds-cache": "down",
                 "general-kernels": "over-backdrop", "four-workgroups": "four-by-three"}
_rules = {}


def _check(rt64_lib, sample_data, name, path="default"):
    case = SC.make_case(sample_data, name)
    kind = case["kind"]
    stats, form = {}, None
    if kind == "primary":
        options, view, form = PRIMARY_PATHS[path]
        sess = SC.gpu_session(rt64_lib, case, options=options, view=view, stats=stats)
    elif kind == "gi":
        sess = SC.gpu_session(rt64_lib, case, options=GI_PATHS[path], stats=stats)
        form = (None, 0 if path == "three-kernel-frame" else 2)          # every gi case is all opaque: its bounce is the wavefront chain (tests/test_gpu_gi_rule.py)
    else:
        options, view = MIRROR_PATHS[path]
        sess, _ = SC.gpu_session(rt64_lib, case, options=options, view=view)
    for f, st in stats.items():
        print("sky_rule %-22s %-20s frame %d leanFrame=%d fusedFrame=%d" % ("gpu/" + path, name, f, st.leanFrame, st.fusedFrame))
        if form is not None:
            assert form[0] in (None, st.leanFrame) and form[1] in (None, st.fusedFrame), (path, name, f, st.leanFrame, st.fusedFrame)
    # Nothing reports which sampler a sky lookup took.  What selects sky_tiled_sample is asserted instead: a frame with GI or reflections, and a sky texture whose
    # sizes are powers of two of 4 and more.  (A 2D lookup -- primary, glass -- always takes the plain sampler.)
    t = np.asarray(case["data_at"](0).textures[case["data_at"](0).sky].data)
    h, w = t.shape[:2]
    random_lookups = kind in ("gi", "mirror")
    assert case["tiled"] == (random_lookups and w >= 4 and h >= 4 and w & (w - 1) == 0 and h & (h - 1) == 0), (name, w, h)
    SC.hold(case, sess, "gpu/" + path, rules=_rules.setdefault(name, {}))
    return case


@pytest.mark.parametrize("name", SC.CASES)
def test_sky_within_the_rule(rt64_lib, sample_data, name):
    case = _check(rt64_lib, sample_data, name)
    if name in ("bounce", "four-by-four", "mirror-floor"):
        assert case["tiled"]                                            # the tiled sampler ...
    if name in ("bounce-padded", "bounce-two-by-two", "glass-sphere"):
        assert not case["tiled"]                                        # ... and the plain one, `bounce-padded` on the texels of `bounce`
    if name == "pole":
        for f in case["compared"]:
            rule = _rules[name][f][0][1]
            poles = rule["sky"] & ~np.isfinite(rule["bound"]).all(axis=-1)
            assert 0 < poles.sum() <= int(SC.UNDECIDED_CAP * rule["sky"].sum()) and not rule["decided"][poles].any()


@pytest.mark.parametrize("path", list(GI_FORMS))
def test_bounce_sky_within_the_rule_on_every_launch_form(rt64_lib, sample_data, path):
    _check(rt64_lib, sample_data, GI_FORMS[path], path)


@pytest.mark.parametrize("path", list(MIRROR_FORMS))
def test_mirror_and_glass_sky_within_the_rule_on_every_launch_form(rt64_lib, sample_data, path):
    _check(rt64_lib, sample_data, MIRROR_FORMS[path], path)


@pytest.mark.parametrize("path", list(PRIMARY_FORMS))
def test_primary_sky_within_the_rule_on_every_launch_form(rt64_lib, sample_data, path):
    _check(rt64_lib, sample_data, PRIMARY_FORMS[path], path)
