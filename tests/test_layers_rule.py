"""The rule of the layered ray queries (tests/layers_rule.py, rules T1-T12) on the CPU: against lists and weights computed by hand, the conditions every case of
tests/layers_cases.py must meet before anything runs on a GPU -- at most 2 % of its rays undecided, at least 32 decided rays with two or more layers in every class of
T5 it is meant for -- and the mutations: each wrong variant of the rule changes the answer on the case named for it, otherwise the cases would not discriminate."""
import numpy as np
import pytest

import layers_cases as LC
import layers_rule as R
import material_rule as M

SEEDS = {name: 100 + k for k, name in enumerate(LC.NAMES)}
# mutation -> the case on which it must change the answer
MUTATION_CASES = {"sorted_by_t": "decal", "no_truncation": "decal", "cutouts_kept": "ignored_hits_8", "opaque_ignores_multiplier": "instances_3",
                  "weights_unquantised": "decal", "glass_does_not_end": "decal", "skipped_layer_scales_rem": "decal", "covered_never_stops": "instances_3"}
Q = lambda k: float(np.float32(k) / np.float32(255.0))


def _rule(sample_data, name, rays, mutate=None):
    data, K, classes = LC.case(sample_data, name)
    o, cand = LC.enumerate_candidates(data, rays)
    try:
        return R.lists(data, M.texture_levels(data), rays, cand, oracle_scene=o, mutate=mutate), classes
    finally:
        o.close()


def _down(x=0.0, z=0.0, y=5.0):
    r = np.zeros((1, 8), dtype=np.float32)
    r[0, 0:3] = (x, y, z); r[0, 4:7] = (0.0, -1.0, 0.0); r[0, 7] = 1000.0
    return r


def test_a_ray_down_through_three_sheets_by_hand(sample_data, oracle_lib):
    """From above: sheet 2 (alpha 0.6), sheet 1 (0.4), sheet 0 (0.2), then the opaque floor, which ends the list.  Instances: the floor is 0, sheet k is 1 + k."""
    rule, _ = _rule(sample_data, "instances_3", _down())
    hits, lay = R.hit_records(rule)
    assert hits.view(np.int32)[:, 0, 3].tolist()[:5] == [3, 2, 1, 0, -1]
    assert lay[0].tolist() == [4, R.LAYERS_VALID | R.LAYERS_ENDS_OPAQUE] and rule["cls"][0] == "a"
    t = hits[:4, 0, 0]
    assert (np.diff(t) > 0).all() and abs(t[3] - 5.0) < 1e-3 and abs(t[2] - (5.0 - (2.3 + 0.004 * 9.9))) < 1e-3
    w = R.weights(rule)
    a = [Q(153), Q(102), Q(51), 1.0]
    want = [a[0], (1 - a[0]) * a[1], (1 - a[0]) * (1 - a[1]) * a[2], (1 - a[0]) * (1 - a[1]) * (1 - a[2])]
    assert np.allclose(w["w"][:4, 0], want, rtol=0, atol=1e-12) and not w["w"][4:, 0].any() and (w["e"][:4, 0] < 1e-6).all()
    assert w["transmittance"][0][0] == 0.0 and w["shaded"][0] == 4 and w["flags"][0] == R.COVERAGE_VALID | R.COVERAGE_COVERED and not w["undecided"][0]
    assert abs(sum(want) - 1.0) < 1e-12
    # maxLayers = 2 writes the first two and says so
    hits2, lay2 = R.hit_records(rule, 2)
    assert hits2.shape[0] == 2 and lay2[0].tolist() == [2, R.LAYERS_VALID | R.LAYERS_ENDS_OPAQUE] and np.array_equal(hits2.view(np.uint32), hits.view(np.uint32)[:2])


def test_the_decal_wins_and_the_glass_takes_the_rest_by_hand(sample_data, oracle_lib):
    """The decal lies 0.02 under the floor and sorts 0.1 in front of it: the list is the 13 sheets from the top, then the decal, and ends there (the floor is behind
    the first opaque entry).  The top sheet is glass of alpha 0.25 -> 64 / 255: it takes 64 / 255, hands the rest to its refracted ray and the resolve stops.
    From below, through ten sheets of 0.6: the sheet of alpha 1 / 255 weighs 0.4^10 / 255 < 1e-6 and is skipped, the sheet behind it sees 0.4^10."""
    rays = np.concatenate([_down(), _down()])
    rays[1, 1] = 1.0; rays[1, 5] = 1.0
    rule, _ = _rule(sample_data, "decal", rays)
    inst = R.hit_records(rule)[0].view(np.int32)[:, :, 3]
    decal, floor = 1 + LC.DECAL_K, 0
    assert inst[:14, 0].tolist() == [1 + k for k in range(12, -1, -1)] + [decal] and inst[14, 0] == -1 and floor not in inst[:, 0]
    assert rule["ends_opaque"][0] and not rule["full"][0]
    w = R.weights(rule)
    assert abs(w["w"][0, 0] - Q(64)) < 1e-12 and not w["w"][1:, 0].any() and abs(w["refraction"][0][0] - (1 - Q(64))) < 1e-12
    assert w["transmittance"][0][0] == 0.0 and w["flags"][0] == R.COVERAGE_VALID | R.COVERAGE_COVERED | R.COVERAGE_GLASS and w["shaded"][0] == 1
    assert inst[:14, 1].tolist() == [1 + k for k in range(13)] + [-1] and not rule["ends_opaque"][1]
    rem = (1 - Q(153)) ** 10
    assert w["w"][LC.FAINT, 1] == 0.0 and abs(w["w"][LC.FAINT + 1, 1] - rem * Q(153)) < 1e-12 and w["shaded"][1] == 12
    assert abs(w["w"][LC.GLASS, 1] - rem * (1 - Q(153)) * Q(64)) < 1e-12 and (w["flags"][1] & R.COVERAGE_GLASS)


@pytest.mark.parametrize("name", LC.NAMES)
def test_every_case_meets_its_conditions(sample_data, oracle_lib, name):
    rays = LC.rays_of(LC.case(sample_data, name)[1], SEEDS[name])
    assert 200 <= len(rays) <= 400
    rule, classes = _rule(sample_data, name, rays)
    w = R.weights(rule)
    cls = np.array(rule["cls"]); length = np.array([len(r) for r in rule["rows"]])
    assert w["undecided"].mean() <= 0.02, float(w["undecided"].mean())
    for c in classes:
        assert ((cls == c) & ~w["undecided"] & (length >= 2)).sum() >= 32, (name, c)
    assert (~rule["valid"]).sum() >= 8 and all(len(rule["rows"][k]) == 0 for k in np.nonzero(~rule["valid"])[0])


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_changes_the_answer_on_its_case(sample_data, oracle_lib, mutation):
    name = MUTATION_CASES[mutation]
    rays = LC.rays_of(LC.case(sample_data, name)[1], SEEDS[name])
    rule, _ = _rule(sample_data, name, rays)
    wrong, _ = _rule(sample_data, name, rays, mutate=mutation)
    # covered_never_stops shows only where something follows complete coverage that a resolve must not read: a record with an out-of-range index
    tail = np.ones(len(rays), dtype=bool) if mutation == "covered_never_stops" else None
    a, b = R.weights(rule, bad_tail=tail), R.weights(wrong, mutate=mutation, bad_tail=tail)
    ha, la = R.hit_records(rule); hb, lb = R.hit_records(wrong)
    differs = (ha.view(np.uint32) != hb.view(np.uint32)).any(axis=(0, 2)) | (la != lb).any(axis=1)
    differs |= (np.abs(a["w"] - b["w"]) > a["e"] + b["e"]).any(axis=0) | (a["flags"] != b["flags"]) | (a["shaded"] != b["shaded"])
    differs |= np.abs(a["transmittance"][0] - b["transmittance"][0]) > a["transmittance"][1] + b["transmittance"][1]
    differs &= ~a["undecided"] & ~b["undecided"]
    assert differs.sum() >= 1, mutation
