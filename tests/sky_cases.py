"""Scene cases of the sky rule tests (tests/test_sky_rule.py on the CPU oracle, tests/test_gpu_sky_rule.py on the GPU) and `hold`, which runs the rule of the pass
that shows the sky -- tests/primary_rule.py, gi_rule.py or mirror_rule.py -- with a sky DESCRIPTION (tests/sky_rule.py) where their own cases have one constant term.

A case is a consumer of the sky (`kind`): "primary" (the pixels a primary ray misses or sees through: SampleSky2D), "gi" (bounce rays that leave the scene:
SampleSkyPlane), "mirror" (mirror rays that leave the scene: SampleSkyPlane) and "glass" (behind a refracting sphere: SampleSky2D at the pixel).  Frames are 88 x 72 as
in tests/gi_cases.py, but for one 4:3 and one 16:9 frame: the aspect ratio enters the plane's UV.

Sky textures are generated from a seed.  The GATED textures keep one channel ordering over the whole image, with a gap of 8 / 255 or more between the channels after
the multiplier (asserted in make_case): a bilinear mix of such texels is convex and keeps the ordering, so no sample lies on ModRGBWithHSL's one discontinuity (g = b
under a red maximum, sky_rule E5) or near a grey.  There is one texture for each of the four branches of RGBtoHCV's two orderings.  The `record-` cases (random channels;
the sample's clouds.png shrunk) are run and their undecided share is written down, not gated.
"""
import copy
import math

import numpy as np

import gi_cases as GC
import gi_rule as G
import light_cases as LC
import mirror_cases as MC
import mirror_rule as M
import primary_cases as PC
import primary_rule as P
import sky_rule as S

W, H = LC.W, LC.H
UNDECIDED_CAP = MC.UNDECIDED_CAP                      # the project's: at most 0.5 % of the pixels that see the sky in the pass

# channels from the largest to the smallest; the branch of (g < b, r < max(g, b)) each one takes
ORDERINGS = {"rgb": (0, 1, 2), "rbg": (0, 2, 1), "grb": (1, 0, 2), "bgr": (2, 1, 0)}
BANDS = ((176, 232), (96, 144), (16, 56))             # bytes of the largest, the middle and the smallest channel
ORDERED_MULTIPLIER = (1.0, 0.875, 1.125)              # keeps every ordering of BANDS: the gaps after it are 10 / 255 and more
PLAIN_MULTIPLIER = (0.5, 0.75, 1.25)                  # with the block off: blue x 1.25 passes 1, and only a modifier that is applied would saturate it
MIN_GAP = 8.0 / 255.0
YAW_OFFSETS = (0.0, -0.83, 7.1)
HSL = {"off": (0.0, 0.0, 0.0), "hue": (0.3, 0.0, 0.0), "saturation": (0.0, -0.25, 0.0), "lightness": (0.0, 0.0, 0.125), "all": (-0.4, 0.2, -0.1),
       "negative-zero": (-0.0, -0.0, -0.0)}


def texture(seed, w, h, ordering, translucent=False):
    """(h, w, 4) bytes from a seed.  ordering: a key of ORDERINGS, or None for three independent channels.  translucent: alpha from 64 up, a quarter of the texels opaque."""
    rng = np.random.default_rng(seed)
    t = np.zeros((h, w, 4), dtype=np.uint8)
    if ordering is None:
        t[..., :3] = rng.integers(16, 241, size=(h, w, 3))
    else:
        for (lo, hi), ch in zip(BANDS, ORDERINGS[ordering]):
            t[..., ch] = rng.integers(lo, hi + 1, size=(h, w))
    t[..., 3] = 255
    if translucent:
        a = rng.integers(64, 255, size=(h, w)); a[rng.random((h, w)) < 0.25] = 255
        t[..., 3] = a
    return t


def padded(t, w, h):
    """The image continued periodically to w x h: the same texels under a size that is no power of two."""
    return np.ascontiguousarray(np.pad(t, ((0, h - t.shape[0]), (0, w - t.shape[1]), (0, 0)), mode="wrap"))


def view_matrix(eye, yaw=0.0, pitch=0.0):
    """World -> view, row vectors, float32: the camera at `eye`, turned by `yaw` about the vertical (as primary_cases._view), then looking up by `pitch`."""
    back = np.array([math.sin(yaw) * math.cos(pitch), -math.sin(pitch), math.cos(yaw) * math.cos(pitch)])
    right = np.array([math.cos(yaw), 0.0, -math.sin(yaw)])
    up = np.cross(back, right)
    r = np.eye(4); r[:3, :3] = np.stack([right, up, back]).T
    t = np.eye(4); t[3, :3] = -np.asarray(eye, dtype=np.float64)
    return (t @ r.astype(np.float32).astype(np.float64)).astype(np.float32)


EYE = (0.0, 2.0, 10.0)
# name -> kind, texture (w, h, ordering | None | "clouds", translucent), multiplier, hsl, yaw offset, then what the kind reads
SPECS = {
    # -- primary: camera, size, upscaler, background instance
    "level":          dict(kind="primary", tex=(64, 32, "bgr"), mult=PLAIN_MULTIPLIER, hsl="off", yaw=0.0, views=[(EYE, 0.4, 0.0)]),
    "up":             dict(kind="primary", tex=(16, 8, "rgb"), mult=ORDERED_MULTIPLIER, hsl="hue", yaw=0.0, views=[(EYE, 0.4, 1.4)]),
    "down":           dict(kind="primary", tex=(16, 8, "rbg"), mult=ORDERED_MULTIPLIER, hsl="saturation", yaw=0.0, views=[((0.0, 6.0, 10.0), -0.7, -1.4)]),
    "seam":           dict(kind="primary", tex=(12, 5, "grb"), mult=ORDERED_MULTIPLIER, hsl="lightness", yaw=0.0, views=[(EYE, -0.02, 0.1), (EYE, 0.02, 0.1)]),
    "jittered":       dict(kind="primary", tex=(64, 32, "bgr"), mult=ORDERED_MULTIPLIER, hsl="all", yaw=-0.83, upscaler=True,
                           views=[(EYE, 0.0, 0.2), ((0.5, 2.0, 10.0), 0.03125, 0.2), ((1.25, 2.25, 9.5), 0.09375, 0.2), ((1.5, 2.25, 9.5), 0.125, 0.2)]),
    "four-by-three":  dict(kind="primary", tex=(4, 4, "rgb"), mult=ORDERED_MULTIPLIER, hsl="all", yaw=7.1, size=(96, 72), views=[(EYE, 0.4, 0.3)]),
    "sixteen-by-nine": dict(kind="primary", tex=(64, 32, "rbg"), mult=ORDERED_MULTIPLIER, hsl="hue", yaw=-0.83, size=(128, 72), views=[(EYE, 2.0, 0.3)]),
    "two-by-two":     dict(kind="primary", tex=(2, 2, "grb"), mult=ORDERED_MULTIPLIER, hsl="saturation", yaw=7.1, views=[(EYE, -1.0, 0.5)]),
    "one-texel":      dict(kind="primary", tex=(1, 1, "bgr"), mult=ORDERED_MULTIPLIER, hsl="all", yaw=-0.83, views=[(EYE, 0.4, 0.3)]),
    "negative-zero":  dict(kind="primary", tex=(16, 8, "bgr"), mult=PLAIN_MULTIPLIER, hsl="negative-zero", yaw=7.1, views=[(EYE, 0.4, 0.3)]),
    "over-backdrop":  dict(kind="primary", tex=(16, 8, "rgb", True), mult=ORDERED_MULTIPLIER, hsl="all", yaw=-0.83, backdrop=True, views=[(EYE, 0.4, 0.3)] * 2),
    "record-mixed":   dict(kind="primary", tex=(64, 32, None), mult=ORDERED_MULTIPLIER, hsl="all", yaw=-0.83, views=[(EYE, 0.4, 0.3)], gated=False),
    "record-clouds":  dict(kind="primary", tex=(64, 32, "clouds"), mult=(1.0, 1.0, 1.0), hsl="all", yaw=0.0, views=[(EYE, 0.4, 0.3)], gated=False),
    # -- gi: samples, bounces, floor tilted or not, background instance
    "bounce":         dict(kind="gi", tex=(64, 32, "rgb"), mult=ORDERED_MULTIPLIER, hsl="all", yaw=-0.83, samples=2, bounces=1),
    "bounce-padded":  dict(kind="gi", tex=(64, 32, "rgb"), pad=(67, 35), mult=ORDERED_MULTIPLIER, hsl="all", yaw=-0.83, samples=2, bounces=1),
    "bounce-off":     dict(kind="gi", tex=(16, 8, "bgr"), mult=PLAIN_MULTIPLIER, hsl="off", yaw=0.0, samples=1, bounces=1),
    "two-bounces":    dict(kind="gi", tex=(16, 8, "rbg"), mult=ORDERED_MULTIPLIER, hsl="saturation", yaw=7.1, samples=1, bounces=2),
    "four-by-four":   dict(kind="gi", tex=(4, 4, "grb"), mult=ORDERED_MULTIPLIER, hsl="lightness", yaw=7.1, samples=1, bounces=1),
    "bounce-two-by-two": dict(kind="gi", tex=(2, 2, "bgr"), mult=ORDERED_MULTIPLIER, hsl="hue", yaw=-0.83, samples=1, bounces=1),
    "pole":           dict(kind="gi", tex=(16, 8, "rgb"), mult=ORDERED_MULTIPLIER, hsl="hue", yaw=0.0, samples=1, bounces=1, level_floor=True),
    "bounce-over-backdrop": dict(kind="gi", tex=(16, 8, "bgr", True), mult=ORDERED_MULTIPLIER, hsl="lightness", yaw=-0.83, samples=1, bounces=1, backdrop=True),
    # -- mirror, glass
    "mirror-floor":   dict(kind="mirror", tex=(16, 8, "rgb"), mult=ORDERED_MULTIPLIER, hsl="hue", yaw=7.1),
    "glass-sphere":   dict(kind="glass", tex=(12, 5, "grb"), mult=ORDERED_MULTIPLIER, hsl="lightness", yaw=-0.83),
}
CASES = tuple(SPECS)
assert {s["yaw"] for s in SPECS.values()} == set(YAW_OFFSETS) and {s["hsl"] for s in SPECS.values()} == set(HSL)
GATED = tuple(n for n in CASES if SPECS[n].get("gated", True))
# the fewest pixels (rays, for gi) that must see the sky over the compared frames: half of what the rule counts in the CPU run of the oracle
# (profiles/sky_rule_deviation.txt records the counts)
SKY_SHARE = {"level": 1721, "up": 3168, "down": 1005, "seam": 4142, "jittered": 9984, "four-by-three": 3181, "sixteen-by-nine": 4608, "two-by-two": 3168, "one-texel": 2930,
             "negative-zero": 2930, "over-backdrop": 2930, "record-mixed": 2930, "record-clouds": 2930, "bounce": 2278, "bounce-padded": 2278, "bounce-off": 2215,
             "two-bounces": 1134, "four-by-four": 2215, "bounce-two-by-two": 2215, "pole": 2699, "bounce-over-backdrop": 1630, "mirror-floor": 590, "glass-sphere": 419}

# the case built to catch each wrong variant of tests/sky_rule.py
MUTATION_CASE = {
    "yaw_offset_ignored": "sixteen-by-nine", "yaw_offset_on_background": "bounce-over-backdrop", "pitch_sign": "up", "aspect_ignored": "sixteen-by-nine",
    "jitter_not_in_sky_uv": "jittered", "clamp_instead_of_wrap": "bounce", "nearest_instead_of_linear": "level", "tile_row_stride": "bounce",
    "multiplier_after_hsl": "jittered", "hsl_when_zero": "bounce-off", "hue_wrapped": "four-by-three", "saturation_on_lightness": "two-bounces", "alpha_modified": "over-backdrop",
    "sky_alpha_ignored": "over-backdrop", "shortcut_below_one": "bounce-over-backdrop",
}


def _tilted(angle_x, angle_z):
    """A rotation by a few degrees about x, then z (row vectors, float32): the floor's normal leaves the vertical, and no bounce ray is exactly vertical."""
    cx, sx, cz, sz = math.cos(angle_x), math.sin(angle_x), math.cos(angle_z), math.sin(angle_z)
    rx = np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]]); rz = np.array([[cz, sz, 0], [-sz, cz, 0], [0, 0, 1]])
    m = np.eye(4, dtype=np.float32); m[:3, :3] = (rx @ rz).astype(np.float32)
    return m


def sky_texels(sample_data, spec):
    w, h, ordering = spec["tex"][:3]
    if ordering == "clouds":
        t = np.asarray(sample_data.textures[sample_data.sky].data)
        t = np.ascontiguousarray(t[::t.shape[0] // h, ::t.shape[1] // w][:h, :w])
    else:
        t = texture(sum(map(ord, "".join(map(str, spec["tex"])))), w, h, ordering, translucent=len(spec["tex"]) > 3)
    if "pad" in spec:
        t = padded(t, *spec["pad"])
    return t


def make_case(sample_data, name):
    """A case dict as the kind's own case module makes them (primary_cases / gi_cases / mirror_cases), with kind, spec, sky_described = True, tiled (the frame has GI or
    reflections and the texture can be tiled: the condition under which the device samples the tiled copy) and gated."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    spec = SPECS[name]
    kind = spec["kind"]
    if kind == "primary":
        d, sphere, floor = MC._base(sample_data)
        floor.material.reflectionFactor = 0.0
        views = [view_matrix(*v) for v in spec["views"]]
        case = dict(name=name, view=dict(di_samples=0, max_lights=12), frames=len(views), compared=tuple(range(len(views))), upscaler=bool(spec.get("upscaler")),
                    background=bool(spec.get("backdrop")))
        if "size" in spec:
            case["size"] = spec["size"]
        if spec.get("backdrop"):
            PC._add_background(d, sample_data); case["compared"] = (1,)
        if spec.get("upscaler"):
            floor.material.lockMask = 0.25; sphere.material.lockMask = 0.75

        def data_at(frame):
            c = copy.copy(d); c.view = views[frame]
            return c
        case["data_at"] = data_at; case["reproject_at"] = lambda f: True
    elif kind == "gi":
        base = "background" if spec.get("backdrop") else "opaque-%d" % spec["samples"]
        case = GC.make_case(sample_data, base)
        d = case["data_at"](0)
        case["bounces"] = spec["bounces"]
        if spec["bounces"] == 2:
            case["compared"] = (1,)
        if not spec.get("level_floor"):
            floor = next(i for i in d.instances if i.name == "floor")
            floor.transform = floor.previous_transform = _tilted(math.radians(2.0), math.radians(3.0))
    else:
        case = MC.make_case(sample_data, "floor" if kind == "mirror" else "glass")
        d = case["data_at"](0)
        if kind == "mirror":
            case["passes"] = 1
    case["name"] = name
    t = sky_texels(sample_data, spec)
    d.textures = list(d.textures)
    d.textures.append(sample_scene.TextureData("sky-" + name, rt64.TEXTURE_FORMAT_RGBA8, t, t.shape[1], t.shape[0])); d.sky = len(d.textures) - 1
    V3 = type(d.desc.skyDiffuseMultiplier)
    d.desc.skyDiffuseMultiplier = V3(*spec["mult"]); d.desc.skyHSLModifier = V3(*HSL[spec["hsl"]]); d.desc.skyYawOffset = spec["yaw"]
    gated = spec.get("gated", True)
    if gated and spec["tex"][2] is not None:                          # the ordering survives the multiplier with a gap
        v = np.sort(t[..., :3].astype(np.float64) / 255.0 * np.asarray(spec["mult"], dtype=np.float32).astype(np.float64), axis=-1)
        order = np.argsort(t[..., :3].astype(np.float64) * np.asarray(spec["mult"]), axis=-1).reshape(-1, 3)
        assert (order == order[0]).all() and np.diff(v, axis=-1).min() >= MIN_GAP and 0.5 * (v[..., 0] + v[..., 2]).max() < 1.0, name
    case.update(kind=kind, spec=spec, sky_described=True, gated=gated, tiled=kind in ("gi", "mirror") and S.can_tile(t))
    return case


# ---- sessions and rules ------------------------------------------------------------------------------------------------------------------------------------

def oracle_session(case):
    k = case["kind"]
    if k == "primary":
        return PC.oracle_session(case)
    if k == "gi":
        return GC.oracle_session(case)
    return MC.oracle_sessions(case)


def gpu_session(rt64_lib, case, options=None, view=None, stats=None):
    """The session on the device.  stats: receives {frame: FRAME_STATS} (primary and gi)."""
    k = case["kind"]
    if k == "primary":
        return PC.gpu_session(rt64_lib, case, options=options, view=view, stats=stats)
    if k == "gi":
        assert view is None
        return GC.gpu_session(rt64_lib, case, options=options, stats=stats)
    return MC.gpu_sessions(rt64_lib, case, options=options, view=view)


def _arm(scene, case, mutate):
    scene["sky"]["mutate"] = mutate; scene["sky"]["tiled"] = case["tiled"]
    return scene


def run_rule(case, frame, sess, mutate=None):
    """The rule of the case's pass for one compared frame, with the sky description armed with a wrong variant of tests/sky_rule.py (or None).
    Returns the pass's rule result with `sky` ((H, W) bool: the pixels that see the sky in the pass)."""
    assert mutate is None or mutate in S.MUTATIONS + S.EQUIVALENT, mutate
    k = case["kind"]
    if k == "primary":
        scene, cam = PC.rule_inputs(case, frame, sess[frame]["background"] if case["background"] else None)
        rule = PC.with_tables(P.primary(_arm(scene, case, mutate), cam), scene)
        rule["sky"] = rule["info"]["coverage"] < 1.0
    elif k == "gi":
        img = sess[frame]
        scene = _arm(GC.rule_scene(case, frame, img["background"]), case, mutate)
        scene["skySeen"] = np.zeros(np.asarray(img["id"]).shape, dtype=bool)
        rule = G.indirect(scene, img["position"], img["normal"], img["id"])
        rule["sky"] = scene["skySeen"]
    else:
        a = sess[(0, frame)]
        scene = _arm(MC.rule_scene(case["data_at"](frame), case["view"], frame, sky_described=True), case, mutate)
        if k == "mirror":
            rule = M.reflection_pass(scene, a["position"], a["view"], a["normal"], a["id"], a["reflection"])
        else:
            pristine = a["refraction"].copy(); pristine[..., :3] = 0.0
            rule = M.refraction_pass(scene, a["position"], a["view"], a["normal"], a["id"], pristine)
        rule["sky"] = rule["info"]["sky"]
    return rule


def judge(case, rule, sess, frame):
    """dict(bad, ratio, undecided, sky): pixels outside the rule, the largest ratio |stored - rule| / bound over decided pixels, undecided pixels among those that see
    the sky, pixels that see the sky."""
    k = case["kind"]
    if k == "primary":
        j = PC.judge(rule, sess[frame])
        bad = int(j["bad"].sum())
        # DIFFUSE holds the sky.  The rule allows the bytes lo .. hi: the stored byte's distance from the middle of that interval over half its width (+ half a
        # byte, the storage step) is below 1 exactly where the byte is allowed.  Every other image of the frame is held to primary_rule as well: `bad` counts them.
        dec = rule["decided"]
        byte = np.rint(np.asarray(sess[frame]["diffuse"], dtype=np.float64) * 255.0)
        lo, hi = rule["diffuse_lo"], rule["diffuse_hi"]
        r = (np.abs(byte - 0.5 * (lo + hi)) / (0.5 * (hi - lo) + 0.5)).max(axis=-1)
        ratio = float(r[dec].max())
    elif k == "gi":
        j = GC.judge(rule, sess[frame])
        bad, ratio, dec = j["bad"], j["ratio"], rule["decided"]
    elif k == "mirror":
        j = MC.judge_pass(rule, sess[(0, frame)], sess[(1, frame)])
        bad, ratio, dec = j["bad"], max(j["ratio"], *j["state"].values()), rule["decided"]
    else:
        j = MC.judge_glass(rule, sess[(0, frame)]["refraction"])
        bad, ratio, dec = j["bad"], j["ratio"], rule["decided"]
    sky = rule["sky"]
    return dict(bad=int(bad), ratio=float(ratio), undecided=int((~dec & sky).sum()), undecided_all=int((~dec).sum()), sky=int(sky.sum()))


def inputs_of(case, sess, frame):
    """The stored bytes the rule of a frame reads: a launch form that stores the same ones is held to the same rule result."""
    k = case["kind"]
    if k == "primary":
        return {"background": sess[frame]["background"]}
    if k == "gi":
        return {key: sess[frame][key] for key in GC.INPUTS}
    return {key: sess[(0, frame)][key] for key in MC.STATE + (("reflection",) if k == "mirror" else ("refraction",))}


def _same(a, b):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()) for k in a)


def hold(case, sess, side, rules=None, log=print):
    """Every compared frame of a session against the rule; asserts the conditions of the tests (a gated case: nothing outside, ratio < 1, undecided within the cap among
    the pixels that see the sky, enough of those) and returns the report rows.  rules: a cache {frame: [(inputs, rule result)]} filled here."""
    rules = {} if rules is None else rules
    name = case["name"]
    rows, seen = [], 0
    for f in case["compared"]:
        inputs = inputs_of(case, sess, f)
        known = [r for i, r in rules.setdefault(f, []) if _same(i, inputs)]
        if not known:
            rules[f].append((inputs, run_rule(case, f, sess)))
            known = [rules[f][-1][1]]
        j = judge(case, known[0], sess, f)
        seen += j["sky"]
        rows.append("sky_rule %-22s %-20s %-7s frame %d ratio=%.6f bad=%d sky=%d undecided=%d (%.3f %%)%s"
                    % (side, name, case["kind"], f, j["ratio"], j["bad"], j["sky"], j["undecided"], 100.0 * j["undecided"] / max(j["sky"], 1),
                       "" if case["gated"] else "  recorded, not gated"))
        log(rows[-1])
        if case["gated"]:
            assert j["bad"] == 0 and j["ratio"] < 1.0, (name, f, j)
            assert j["undecided"] <= int(UNDECIDED_CAP * j["sky"]), (name, f, j)
    assert seen >= SKY_SHARE.get(name, 1), (name, seen)
    return rows
