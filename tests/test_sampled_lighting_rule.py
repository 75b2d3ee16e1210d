"""tests/sampled_lighting_rule.py pinned on the CPU (rules J1-J11).  No CPU path makes sampled-lighting records, so the rule is pinned to the
picture instead: at a frame's stored G-buffer with keys (px, py, frameCount) its direct + emitted is light_rule.direct_light's value (the join is the same) and
lies within L8 of the oracle's DIRECT_LIGHT_RAW; its own evaluation of every case of tests/sampled_lighting_cases.py stays under the undecided cap for the keys
chosen there; hand-worked walks, noise factors, a miss and two bad hits; and each named wrong reading leaves the bound on its case, against the rule's own records,
on more records than the case leaves undecided.
"""
import json
import os

import numpy as np
import pytest

import light_cases as LC
import light_rule as L
import material_rule as M
import sampled_lighting_cases as SC
import sampled_lighting_rule as R
from test_oracle_kats import GOLD, _tea

PICTURE_UNDECIDED_CAP = 0.005          # L9's
_cases, _rules = {}, {}


def _case(sample_data, name):
    """(scene, view, frames, rays, keys, the oracle's hits, texture levels) of a case, made once."""
    if name not in _cases:
        data, view, frames = SC.make_case(sample_data, name)
        rays, keys = SC.rays_and_keys(data, name)
        _cases[name] = (data, view, frames, rays, keys, SC.oracle_hits(data, rays), M.texture_levels(data))
    return _cases[name]


def _rule(sample_data, name, overrides=(-1, -1), mutate=None):
    key = (name, overrides, mutate)
    if key not in _rules:
        data, view, frames, rays, keys, hits, levels = _case(sample_data, name)
        _rules[key] = R.sampled(data, levels, rays, hits, keys, SC.frame_of(view, frames), max_lights=overrides[0], di_samples=overrides[1], mutate=mutate)
    return _rules[key]


# ---- the rule's own evaluation of the cases ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SC.NAMES)
def test_the_rule_decides_the_cases(sample_data, oracle_lib, name):
    """For the keys chosen the rule leaves at most 2 % of a case's real hits undecided, the case shows what it was built to show, and every frame value of the case
    has records."""
    rule = _rule(sample_data, name)
    ratios, exact = R.compare(rule, R.as_records(rule))
    print(R.report(name, rule, ratios, exact))
    real = rule["kind"] == 2
    sh = R.shares(rule)
    assert real.sum() >= 300 and exact.all() and all((r <= 1.0).all() for r in ratios.values())
    assert sh[3] <= SC.UNDECIDED_CAP, sh
    assert all(a >= b for a, b in zip(sh[:3], SC.SHARES[name])), (sh, SC.SHARES[name])
    keys = _case(sample_data, name)[4]
    for f in SC.FRAMES[name]:
        assert (real & (keys[:, 2] == f)).sum() >= 5, f
    assert (keys[:, 0] >= 64).sum() > 500 and (keys[:, 1] >= SC.H).sum() > 500          # keys off the noise tile and off the frame


def test_the_overrides_change_the_records(sample_data, oracle_lib):
    """J4 on "four" (3 lights, 2 samples): {16, 0} draws every candidate once at its centre -- popcount(drawn) = lightsAdmitted where no slot is reached twice --
    and a field of -1 keeps the frame's value."""
    base, over = _rule(sample_data, "four"), _rule(sample_data, "four", SC.OVERRIDES["four"])
    real = (base["kind"] == 2) & ~base["undecided"] & ~over["undecided"]
    assert (base["draws"][real] == np.minimum(base["admitted"][real], 3)).all() and (over["draws"][real] == over["admitted"][real]).all()
    once = real & ((over["drawn"] >> 16) == 0)
    pop = np.array([bin(int(x) & 0xFFFF).count("1") for x in over["drawn"]])
    assert once.sum() > 0.9 * real.sum() and (pop[once] == over["admitted"][once]).all()
    data, view, frames, rays, keys, hits, levels = _case(sample_data, "four")
    part = slice(2800, 3000)
    half = R.sampled(data, levels, rays[part], hits[part], keys[part], SC.frame_of(view, frames), max_lights=-1, di_samples=2)
    assert (half["kind"] == 2).sum() > 100 and np.array_equal(R.as_records(half).view(np.uint32), R.as_records(base).view(np.uint32)[part])


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_wrong_readings_leave_the_bound(sample_data, oracle_lib, mutation):
    name = SC.MUTATION_CASE[mutation]
    overrides = SC.OVERRIDES[name] if mutation == "overrides_ignored" else (-1, -1)
    rule = _rule(sample_data, name, overrides)
    wrong = _rule(sample_data, name, overrides, mutation)
    out = R.outside(wrong, R.as_records(rule))
    und = int((wrong["undecided"] | rule["undecided"]).sum())
    print("mutation %-22s on %-9s %4d of %4d of the rule's own records outside its bound (undecided with either: %d)" % (mutation, name, int(out.sum()), len(out), und))
    assert out.sum() > und, mutation


# ---- the picture (J10) -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SC.NAMES)
def test_the_rule_is_the_picture_at_stored_inputs(sample_data, oracle_lib, name):
    """The oracle's own G-buffer goes through this rule with keys (px, py, frameCount) and through light_rule.direct_light: the same join, so the two values agree
    within the sum of their errors (in fact far closer), both decide the same pixels, and the oracle's DIRECT_LIGHT_RAW lies within L8 of this rule.  The oracle's
    binding draws every instance with the scene's shader, so the "noise" case is drawn without its noise option here (the GPU test draws it with)."""
    from oracle import oracle_py
    d, view, frames = SC.make_case(sample_data, name)
    for i in d.instances:
        i.shader = None
    o = oracle_py.OracleScene(d)
    try:
        for f in range(frames):
            ref = o.render(SC.W, SC.H, images=(f == frames - 1), diSamples=view["di_samples"], maxLights=view["max_lights"])
    finally:
        o.close()
    theirs, their_bound, their_decided, info = LC.run_rule(d, view, frames - 1, ref["shadingPosition"], ref["shadingNormal"], ref["shadingSpecular"], ref["instanceId"])
    mine, bound, decided, drawn = R.at_gbuffer(d, ref["shadingPosition"], ref["shadingNormal"], ref["shadingSpecular"], ref["instanceId"], LC.rule_inputs(d)["camera"],
                                               SC.frame_of(view, frames))
    lit = ref["instanceId"] >= 0
    assert np.array_equal(decided[lit], their_decided[lit])
    both = lit & decided
    diff = np.abs(mine - theirs[..., :3])
    assert (diff[both] <= (bound + their_bound[..., :3])[both]).all()
    stored = np.abs(ref["directLight"][..., :3].astype(np.float64) - mine)
    left_out = 1.0 - both.sum() / lit.sum()
    pop = np.array([bin(int(x) & 0xFFFF).count("1") + bin(int(x) >> 16).count("1") for x in drawn.reshape(-1)]).reshape(drawn.shape)
    print("%-9s shaded %4d  left out %.4f  |rule - light_rule| max %.2e  |oracle - rule| / L8 max %.3f" %
          (name, int(lit.sum()), left_out, diff[both].max(), (stored[both] / bound[both]).max()))
    assert lit.sum() > 1500 and left_out <= PICTURE_UNDECIDED_CAP
    assert (stored[both] <= bound[both]).all()
    assert (pop[both] == info["draws"][both]).all()          # every draw sets one bit


# ---- hand-worked records -----------------------------------------------------------------------------------------------------------------------------------------------

def _walk(intensities, bytes_, max_lights, **kw):
    n = len(intensities)
    col = np.zeros((1, 16)); col[0, :n] = intensities
    idx = np.zeros((1, 16), dtype=np.int64); idx[0, :n] = [7, 3, 9, 12][:n]
    noise = np.array([[b / 255.0] for b in bytes_])
    return int(R.drawn_mask(col, idx, np.array([n]), noise, max_lights, **kw)[0])


def test_two_candidates_and_every_branch_of_the_walk():
    """Candidates 3 and 1 (total 4).  Draw 0: r = byte / 255 * 4 against the running sum 3: a byte of 191 gives 2.996 < 3 -> slot 0, 192 gives 3.012 >= 3 -> slot 1 (the
    walk stops at the last slot whatever r is).  Draw 1 walks the zeroed column."""
    assert _walk([3.0, 1.0], [191], 1) == 0b01 and _walk([3.0, 1.0], [192], 1) == 0b10 and _walk([3.0, 1.0], [255], 1) == 0b10
    # slot 0 drawn and zeroed: remaining 1, running sum 0, so any r >= 0 walks on to slot 1
    assert _walk([3.0, 1.0], [0, 0], 2) == 0b11 and _walk([3.0, 1.0], [100, 255], 2) == 0b11
    # slot 1 drawn first (remaining 3): r = byte / 255 * 3 < 3 stays at slot 0 for every byte but 255 ...
    assert _walk([3.0, 1.0], [200, 254], 2) == 0b11
    # ... and a byte of 255 gives r = 3 >= 3: the walk reaches slot 1 again after it was zeroed (the frame lights that candidate twice and never slot 0)
    assert _walk([3.0, 1.0], [200, 255], 2) == 0b10 | (0b10 << 16)
    assert _walk([3.0, 1.0], [200, 255], 2, zeroing=False) == 0b10 | (0b10 << 16)          # (not zeroed: r = 255 / 255 * 3 >= 3 as well)
    assert _walk([3.0, 1.0], [200, 254], 2, zeroing=False) == 0b11
    assert _walk([3.0, 1.0], [0, 0], 2, zeroing=False) == 0b01 | (0b01 << 16)              # not zeroed: slot 0 both times
    assert _walk([3.0, 1.0], [192], 1, by_index=True) == 1 << 3                            # the wrong reading: the light's index
    assert _walk([3.0, 1.0], [192], 0) == 0 and _walk([5.0], [255], 1) == 0b01 and _walk([5.0], [255], 0) == 0
    assert _walk([1.0, 1.0, 1.0, 1.0], [0, 0, 0, 0], 12) == 0b1111                         # four draws of a byte 0: the first slot left each time


def test_the_noise_factor_is_the_pinned_hash():
    """J8: rint(next_rand(init_rand(x + y * width, frame, 16))) against tests/golden/kats.json and test_oracle_kats._tea, a factor of 0 and of 1 among them."""
    kats = json.load(open(os.path.join(GOLD, "kats.json")))["init_rand"]
    seen = set()
    for k in kats:
        assert int(R.init_rand(np.array([k["val0"]]), np.array([k["val1"]]))[0]) == k["seed"] == _tea(k["val0"], k["val1"])
        want = int(np.rint(np.float32(k["next"][0])))
        x, y, width = k["val0"] % 88, k["val0"] // 88, 88
        assert int(R.noise_factor(np.array([x]), np.array([y]), np.array([k["val1"]]), width)[0]) == want
        seen.add(want)
    f = R.noise_factor(np.arange(4096) % 64, np.arange(4096) // 64, np.full(4096, 5), 88)
    assert seen <= {0, 1} and set(f.tolist()) == {0, 1} and 0.4 < f.mean() < 0.6
    # x + y * width wraps in 32 bits, and only the sum matters
    assert int(R.noise_factor(np.array([2 ** 32 - 1]), np.array([1]), np.array([9]), 88)[0]) == int(R.noise_factor(np.array([87]), np.array([0]), np.array([9]), 88)[0])
    assert int(R.noise_factor(np.array([88]), np.array([0]), np.array([9]), 88)[0]) == int(R.noise_factor(np.array([0]), np.array([1]), np.array([9]), 88)[0])


def test_one_disc_sample_by_hand():
    """L4 at one sample: the light straight above the point, so perpX = (1, 0, 0) and perpY = cross(perpX, -L) = (0, 0, -1); a table of bytes (255, 0): the disc
    vector (1, -1) normalised times saturate(sqrt 2) = (0.7071, -0.7071); radius 2 moves the sample to (1.4142, 5, 1.4142) -- distance sqrt(29), against 5 at
    diSamples = 0, where the radius does not count."""
    table = np.zeros((512, 512, 4), dtype=np.uint8); table[..., 0] = 255
    light = dict(position=(0.0, 5.0, 0.0), diffuseColor=(1.0, 1.0, 1.0), attenuationRadius=10.0, pointRadius=2.0, specularColor=(0.0, 0.0, 0.0), shadowOffset=0.0,
                 attenuationExponent=1.0, groupBits=1)
    clear = lambda o, d, tmin, tmax, a, b: np.ones(len(o), dtype=np.int8)
    st = {"position": L.vec(np.zeros((1, 3))), "normal": L.vec(np.array([[0.0, 1.0, 0.0]])), "specular": L.vec(np.ones((1, 3))), "rayDirection": L.vec(np.array([[0.0, -1.0, 0.0]])),
          "px": np.array([70]), "py": np.array([3]), "bluenoise": table, "frameCount": 63, "shadow": clear,
          "ignoreNormalFactor": np.zeros(1), "specularExponent": np.ones(1), "shadowRayBias": np.zeros(1)}
    got = {ds: L.light_loop(dict(st, diSamples=ds), np.array([1], dtype=np.uint32), [light], 1)[0][0].v[0] for ds in (0, 1)}
    assert abs(got[0] - 0.5) < 1e-12                                            # N.L = 1, falloff 1 - 5 / 10
    d = np.sqrt(29.0)
    assert abs(got[1] - (5.0 / d) * (1.0 - d / 10.0)) < 1e-9


def test_a_miss_and_two_bad_hits(sample_data, oracle_lib):
    """J1: the miss record and the two bad-hit records (instance past the end, primitive past the end), word for word; nothing else of the batch moves."""
    data, view, frames, rays, keys, hits, levels = _case(sample_data, "pick-one")
    real = np.nonzero(hits.view(np.int32)[:, 3] >= 0)[0][:40]
    r, h, k = rays[real].copy(), hits[real].copy(), keys[real].copy()
    hb = h.view(np.uint32)
    hb[1, 3] = 0xFFFFFFFF; hb[2, 3] = 1000; hb[3, 4] = 0x7FFFFFFF
    rule = R.sampled(data, levels, r, h, k, SC.frame_of(view, frames))
    rec = R.as_records(rule).view(np.uint32)
    assert rule["kind"].tolist()[:5] == [2, 0, 1, 1, 2]
    for row, flags in ((1, 0), (2, R.BAD_HIT), (3, R.BAD_HIT)):
        want = np.zeros(16, dtype=np.uint32); want[3] = flags; want[12] = want[13] = 0xFFFFFFFF
        assert np.array_equal(rec[row], want)
    whole = R.as_records(R.sampled(data, levels, rays[real], hits[real], keys[real], SC.frame_of(view, frames))).view(np.uint32)
    keep = np.ones(len(real), dtype=bool); keep[1:4] = False
    assert np.array_equal(rec[keep], whole[keep]) and (rec[keep][:, 3] & R.VALID).all()
