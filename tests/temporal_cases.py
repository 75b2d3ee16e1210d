"""Cases of the temporal-accumulation rule tests (tests/test_temporal_rule.py on the CPU oracle, tests/test_gpu_temporal_rule.py on the GPU), the twin sessions both
draw, and `hold`, which compares INDIRECT_LIGHT_RAW and GI_MOMENTS of every compared frame with tests/temporal_rule.py.

A case is a sequence of frames of a gi_cases scene (lights, materials and geometry as gi_cases sets them up: `opaque-1`, or `layers` for the per-pixel hit lists)
drawn with GI and the denoiser ON, 88 x 72 unless the case sets a size.  For every compared frame N two sessions draw the same calls: A, the session under test, and
a twin B_N whose frame N alone has denoiserEnabled = 0 (temporal_rule.py says why that makes B's frame N the fresh radiance).  Both read back frames N - 1 and N.
A case asserts from the rule's own counts that it contains what it was built for (SHARES: half of what the CPU oracle shows, profiles/temporal_rule_deviation.txt)."""
import copy
import math

import numpy as np

import gi_cases as GC
import mirror_cases as MC
import primary_cases as PC
import temporal_rule as T

W, H = GC.W, GC.H
UNDECIDED_CAP = 0.001             # at most 0.1 % of a frame's surface pixels may be undecided (N1: only a flow the check of the float32 sum refuses)

CASES = ("static", "cap", "strafe-left", "strafe-right", "turning", "vertical", "no-reproject", "layers", "two-samples", "two-bounce", "gaussian", "ragged")

# Minimum counts over the compared frames (temporal_rule.accumulate's info), half of what the oracle shows.  above_one / below_one: weights over 1 / in (0.95, 1);
# intermediate: weights in (0.05, 0.95); disoccluded: previous pixel inside the frame, weight under 1e-3; truncation_x / _y: x + 0.5 + flow.x (y ...) in (-1, 0);
# off_*: previous pixel past that edge; capped: history 64 after the frame; capped_before: previous history already 64; fixed_point: history in (32, 64) (the
# fixed point h = h w + 1 of a weight just under 1); grown: history up by MORE than one; zero_history: h0 exactly 0; flow_y: flow.y not 0.
SHARES = {
    "static": dict(above_one=865, below_one=759, grown=865),
    "cap": dict(capped=1424, capped_before=1177, fixed_point=97, above_one=197),
    "strafe-left": dict(truncation_x=19, disoccluded=34, intermediate=270, above_one=239, zero_history=36),
    "strafe-right": dict(off_right=19, disoccluded=27, intermediate=259, above_one=249),
    "turning": dict(intermediate=1094, flow_y=1181),
    "vertical": dict(flow_y=6336, off_top=44, off_bottom=176, truncation_y=44, disoccluded=81),
    "no-reproject": dict(intermediate=500, disoccluded=29),
    "layers": dict(truncation_x=32, intermediate=269, disoccluded=32),
    "two-samples": dict(off_right=28, intermediate=394, grown=5112),
    "two-bounce": dict(truncation_x=9, intermediate=135),
    "gaussian": dict(off_right=9, intermediate=127),
    "ragged": dict(intermediate=44, disoccluded=3, below_one=19),
}

# the case built to catch each wrong variant of the rule, and the compared frame it shows in
MUTATION_CASE = {
    "floor_not_trunc": ("strafe-left", 3), "no_half_pixel": ("strafe-left", 3), "flow_subtracted": ("strafe-left", 3), "previous_at_current_pixel": ("strafe-left", 3),
    "edge_clamped_not_zero": ("strafe-right", 3), "depth_scale_tenth": ("strafe-left", 3), "normal_exponent_64": ("turning", 3), "weight_clamped_at_one": ("static", 6),
    "history_unweighted": ("turning", 3), "cap_before_increment": ("cap", 66), "no_cap": ("cap", 66), "moments_at_current_pixel": ("strafe-left", 3),
    "moments_alpha_one": ("static", 3), "alpha_not_history": ("static", 3), "guides_of_current_frame": ("strafe-left", 3),
}

GPU_IMAGES = {"raw": "INDIRECT_LIGHT_RAW", "moments": "GI_MOMENTS", "depth": "DEPTH", "normal": "SHADING_NORMAL", "flow": "FLOW", "id": "INSTANCE_ID",
              "direct": "DIRECT_LIGHT_RAW", "filtered": "INDIRECT_LIGHT_FILTERED"}
ORACLE_IMAGES = {"raw": "indirectLight", "moments": "moments", "depth": "depth", "normal": "shadingNormal", "flow": "flow", "id": "instanceId",
                 "direct": "directLight", "filtered": "filteredIndirect"}
RULE_INPUTS = (("cur", ("flow", "depth", "normal", "id")), ("prev", ("raw", "moments", "depth", "normal")), ("fresh", ("raw", "moments")))
SVGF, GAUSSIAN = 1, 0


def _rotation(axis, angle, centre):
    """Object -> object, row vectors: a turn by `angle` about `axis` through `centre`."""
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    r = np.eye(3) + math.sin(angle) * k + (1.0 - math.cos(angle)) * (k @ k)
    m = np.eye(4); m[:3, :3] = r.T; m[3, :3] = np.asarray(centre) - np.asarray(centre) @ r.T
    return m.astype(np.float32)


def make_case(sample_data, name):
    """dict(name, size, frames, compared, view, bounces, mode, data_at: frame -> SceneData (its view is that frame's camera), reproject_at: frame -> canReproject)."""
    base = GC.make_case(sample_data, "layers" if name == "layers" else "opaque-1")
    d = base["data_at"](0)
    case = dict(name=name, size=(W, H), frames=6, compared=(3, 5), view=dict(di_samples=0, gi_samples=1, max_lights=12), bounces=1, mode=SVGF)
    eye = lambda f: (0.0, 2.0, 10.0)
    insts, reproject = None, {}
    left = lambda f: (-0.06 * f, 2.0, 10.0)
    right = lambda f: (0.06 * f, 2.0, 10.0)
    if name == "static":
        case["frames"] = 7; case["compared"] = (2, 3, 6)
    elif name == "cap":
        case["size"] = (48, 27); case["frames"] = 71; case["compared"] = (63, 64, 65, 66, 70)
    elif name == "strafe-left":
        eye = left
    elif name == "strafe-right":
        eye = right
    elif name == "turning":
        sphere = next(i for i in d.instances if i.name == "sphere"); k = d.instances.index(sphere)
        p = d.meshes[sphere.mesh].vertices["position"][:, :3].astype(np.float64)
        centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
        at = lambda f: _rotation((1.0, 2.0, 0.5), 0.08 * f, centre)
        insts = {}
        for f in range(4):
            l = list(d.instances); l[k] = PC._moved(sphere, at(f), at(max(f - 1, 0))); insts[f] = l
        case["frames"] = 4; case["compared"] = (2, 3)
    elif name == "vertical":
        # up for three frames, then down again: previous rows above the frame, then below it.  A wall behind everything fills the upper rows; at its distance a
        # step of 0.3 is 1.8 pixels: row 0 comes from above the frame, row 1 lies in the truncation window
        MC._add_quad(d, "backdrop", (0.0, 4.0, -4.5), 12.0, 8.0, "camera")
        height = [2.0, 2.3, 2.6, 2.9, 2.6, 2.3]
        eye = lambda f: (0.0, height[f], 10.0)
    elif name == "no-reproject":
        eye = left; reproject = {3: False}; case["frames"] = 5; case["compared"] = (3, 4)
    elif name == "layers":
        eye = left; case["frames"] = 4; case["compared"] = (2, 3)
    elif name == "two-samples":
        eye = right; case["view"]["gi_samples"] = 2; case["frames"] = 5; case["compared"] = (2, 3, 4)
    elif name == "two-bounce":
        eye = left; case["bounces"] = 2; case["frames"] = 3; case["compared"] = (2,)
    elif name == "gaussian":
        eye = right; case["mode"] = GAUSSIAN; case["frames"] = 3; case["compared"] = (2,)
    elif name == "ragged":
        eye = left; case["size"] = (33, 17); case["frames"] = 4; case["compared"] = (2, 3)
    else:
        raise KeyError(name)
    views = [PC._view(eye(f), 0.0) for f in range(case["frames"])]
    if insts is not None:
        d.instances = insts[0]

    def data_at(frame):
        c = copy.copy(d)
        c.view = views[frame]
        if insts is not None:
            c.instances = insts[frame]
        return c
    case["data_at"] = data_at; case["reproject_at"] = lambda f: reproject.get(f, True)
    e = d.desc
    case["ambient"] = ((e.ambientBaseColor.x, e.ambientBaseColor.y, e.ambientBaseColor.z), (e.ambientNoGIColor.x, e.ambientNoGIColor.y, e.ambientNoGIColor.z))
    return case


# ---- sessions ---------------------------------------------------------------------------------------------------------------------------------------

def _frames(case, last):
    now = None
    for f in range(last + 1):
        d = case["data_at"](f)
        changed = [] if now is None else [(j, inst) for j, inst in enumerate(d.instances) if inst is not now[j]]
        now = list(d.instances)
        yield f, d, changed


def _oracle_run(case, last, off_at, wanted):
    from oracle import oracle_py
    out = {}
    o = oracle_py.OracleScene(case["data_at"](0))
    try:
        for f, d, changed in _frames(case, last):
            for j, inst in changed:
                o.set_instance(j, inst)
            o.data = d
            ref = o.render(*case["size"], images=f in wanted, can_reproject=case["reproject_at"](f), diSamples=case["view"]["di_samples"],
                           giSamples=case["view"]["gi_samples"], maxLights=case["view"]["max_lights"], maxReflections=0, giBounces=case["bounces"],
                           denoiserEnabled=0 if f == off_at else 1, denoiserMode=case["mode"])
            if f in wanted:
                assert ref["pixelJitter"] == (0.0, 0.0)
                out[f] = {key: ref[name] for key, name in ORACLE_IMAGES.items()}
    finally:
        o.close()
    return out


def _gpu_run(rt64_lib, case, last, off_at, wanted, options, band, stats):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    out = {}
    s = sample_scene.Rt64Scene(rt64_lib, case["data_at"](0), *case["size"], hip_device=0)
    try:
        s.set_view_description(denoiser=True, **case["view"])
        assert s.option("max_reflections", 0) and s.option("gi_bounces", case["bounces"]) and s.option("denoiser_mode", case["mode"])
        for key, v in (options or {}).items():
            assert s.option(key, v), key
        if band:
            s.set_tile(*band)
        for f, d, changed in _frames(case, last):
            for j, inst in changed:
                s.set_instance(j, inst)
            s.data = d
            if f == off_at:
                s.set_view_description(denoiser=False, **case["view"])
            s.draw(can_reproject=case["reproject_at"](f))
            if f in wanted:
                if stats is not None and off_at is None:
                    stats[f] = s.stats()
                out[f] = {key: s.readback(getattr(rt64, "IMAGE_" + name)) for key, name in GPU_IMAGES.items()}
    finally:
        s.close()
    return out


def _twins(case, run):
    """{N: dict(a_prev, a, b_prev, b)}: session A once, a twin per compared frame."""
    wanted = {f for n in case["compared"] for f in (n - 1, n)}
    a = run(max(case["compared"]), None, wanted)
    out = {}
    for n in case["compared"]:
        b = run(n, n, {n - 1, n})
        out[n] = dict(a_prev=a[n - 1], a=a[n], b_prev=b[n - 1], b=b[n])
    return out


def oracle_session(case):
    return _twins(case, lambda last, off_at, wanted: _oracle_run(case, last, off_at, wanted))


def gpu_session(rt64_lib, case, options=None, band=None, stats=None):
    """The same sessions on the device, with device options (a launch form) and, with `band`, a device that owns rows [y0, y1) only: its readbacks are those
    rows.  stats: a dict that receives {frame: FRAME_STATS} of session A's compared frames."""
    return _twins(case, lambda last, off_at, wanted: _gpu_run(rt64_lib, case, last, off_at, wanted, options, band, stats))


# ---- holding a side to the rule ---------------------------------------------------------------------------------------------------------------------

def rule_inputs(pair):
    return dict(cur={k: pair["a"][k] for k in RULE_INPUTS[0][1]}, prev={k: pair["a_prev"][k] for k in RULE_INPUTS[1][1]},
                fresh={k: pair["b"][k] for k in RULE_INPUTS[2][1]})


def run_rule(case, pair, mutate=None):
    i = rule_inputs(pair)
    return T.accumulate(i["cur"], i["prev"], i["fresh"], case["view"]["gi_samples"], case["ambient"], mutate=mutate)


def _bytes(x):
    return np.ascontiguousarray(x).tobytes()


def inputs_equal(a, b):
    return all(_bytes(a[g][k]) == _bytes(b[g][k]) for g, keys in RULE_INPUTS for k in keys)


def check_twin(case, n, pair, rule):
    """(N8) and the small things around it."""
    name, samples = case["name"], case["view"]["gi_samples"]
    for k in GPU_IMAGES:
        assert _bytes(pair["a_prev"][k]) == _bytes(pair["b_prev"][k]), (name, n, k, "the sessions differ before the compared frame")
    surface = np.asarray(pair["a"]["id"]) >= 0
    for k in ("flow", "depth", "normal", "id", "direct"):
        assert _bytes(pair["a"][k]) == _bytes(pair["b"][k]), (name, n, k, "the twin's frame differs in more than the history")
    assert np.array_equal(np.asarray(pair["b"]["raw"])[..., 3], np.where(surface, float(samples), 0.0)), (name, n, "the twin's alpha is not giSamples")
    # DIRECT_LIGHT_RAW carries no history (diReproject is compiled out): alpha 1 on a surface, 0 elsewhere
    for side in ("a", "b"):
        assert np.array_equal(np.asarray(pair[side]["direct"])[..., 3], np.where(surface, 1.0, 0.0)), (name, n, side, "DIRECT_LIGHT_RAW carries a history")
    # a frame the denoiser does not touch: the filtered image is the raw one
    assert _bytes(pair["b"]["filtered"]) == _bytes(pair["b"]["raw"]), (name, n, "INDIRECT_LIGHT_FILTERED of the twin is not its INDIRECT_LIGHT_RAW")
    # h0 exactly 0: h = 1 and both lerps have t = 1, a + (b - a) * 1 in float32.  That is b bit for bit where a is 0 (every previous pixel off the frame; the moments
    # behind a previous pixel without a surface).  The moments are float32 on both sides, so the expression is evaluated here and must match everywhere; the colour's
    # b is known only as float16, so it must match where the previous colour is 0 and stays inside N4's bound (half a float16 step and a few float32 roundings) elsewhere
    z = rule["zero_history"]
    pm = np.where(rule["inside"][..., None], np.asarray(pair["a_prev"]["moments"], dtype=np.float32)[rule["prev_y"], rule["prev_x"]], np.float32(0.0))[z]
    fm = np.asarray(pair["b"]["moments"], dtype=np.float32)[z]
    assert _bytes(np.asarray(pair["a"]["moments"], dtype=np.float32)[z]) == _bytes(pm + (fm - pm) * np.float32(1.0)), (name, n, "h0 = 0 and the moments are not lerp(previous, fresh, 1)")
    off = z & ~rule["inside"]
    assert _bytes(np.asarray(pair["a"]["moments"])[off]) == _bytes(np.asarray(pair["b"]["moments"])[off]), (name, n, "no previous pixel and the moments are not the fresh ones")
    assert _bytes(np.asarray(pair["a"]["raw"])[off][:, :3]) == _bytes(np.asarray(pair["b"]["raw"])[off][:, :3]), (name, n, "no previous pixel and the colour is not the fresh one")


def judge(rule, pair):
    ratios, bad = T.compare(pair["a"]["raw"], pair["a"]["moments"], rule)
    return dict(ratios=ratios, ratio=max(v[0] for v in ratios.values()), bad=int(bad.sum()), undecided=int((rule["surface"] & ~rule["decided"]).sum()),
                uncovered=int((rule["surface"] & ~rule["covered"]).sum()), surface=int(rule["surface"].sum()))


def hold(case, sessions, side, rules=None, log=print, shares=True):
    """Every compared frame of the twin sessions against the rule; asserts the conditions of the tests and returns the report rows.  rules: a cache
    {frame: [(inputs, rule result)]} filled here: a launch form whose stored inputs are the same bytes reuses the result."""
    rules = {} if rules is None else rules
    name = case["name"]
    rows, total = [], {}
    for n in case["compared"]:
        pair = sessions[n]
        inputs = rule_inputs(pair)
        known = [r for i, r in rules.setdefault(n, []) if inputs_equal(i, inputs)]
        if not known:
            rules[n].append((inputs, run_rule(case, pair)))
            known = [rules[n][-1][1]]
        rule = known[0]
        check_twin(case, n, pair, rule)
        j = judge(rule, pair)
        r = j["ratios"]
        rows.append("temporal_rule %-22s %-13s frame %2d rgb=%.6f/%.6f alpha=%.6f/%.6f moments=%.6f/%.6f surface=%d undecided=%d uncovered=%d counts %s"
                    % (side, name, n, r["rgb"][0], r["rgb"][1], r["alpha"][0], r["alpha"][1], r["moments"][0], r["moments"][1], j["surface"], j["undecided"],
                       j["uncovered"], {k: v for k, v in rule["info"]["counts"].items() if v}))
        log(rows[-1])
        assert j["bad"] == 0 and j["ratio"] < 1.0, (name, n, j)
        assert j["undecided"] <= int(UNDECIDED_CAP * j["surface"]), (name, n, j["undecided"], j["surface"])
        assert j["uncovered"] == 0 or name == "cap", (name, n, j["uncovered"])
        for k, v in rule["info"]["counts"].items():
            total[k] = total.get(k, 0) + v
    for k, need in (SHARES[name] if shares else {}).items():
        assert total.get(k, 0) >= need and total.get(k, 0) > 0, (name, k, total.get(k, 0), need)
    return rows
