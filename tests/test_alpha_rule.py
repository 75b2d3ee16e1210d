"""The rule for ray queries that honour alpha (tests/alpha_rule.py, rules K1-K10 of DESIGN.md 4) checked on the CPU, from the oracle's intersection enumeration.

 * the cases keep their conditions: at most 2 % of the rays undecided (nothing else excludes a ray), at least 100 rays with two or more subtracting candidates on the
   stacked translucent cases, at least 100 rays whose closest candidate is a cutout on the fences;
 * the BVH enumeration yields the candidate multiset of brute force on every case;
 * K8 holds for the rule against the oracle's committing walk (tests/ray_rule.py);
 * K2 for camera rays names the instance the oracle's frame shows at that pixel of the fence;
 * every wrong reading of the rule (`mutate=`) leaves the bound of the right one on a named case -- the counts seen are printed and recorded in MUTATION_MISSES.
"""
import numpy as np
import pytest

import alpha_cases as AC
import alpha_rule as R
import material_cases as MC
import material_rule as M
import ray_rule

W, H = 64, 36
MUTATION_CASES = {
    "cutout_commits": "fence",
    "edge_on_every_shader": "veils",
    "cutout_at_level_0": "mipped fence",
    "shadow_at_given_lod": "mipped fence",
    "shadow_uses_solid_alpha": "fence",
    "o2_ignored": "mixed",
    "stops_at_first_subtraction": "veils",
    "closest_only": "veils",
    "shadow_cutout_subtracts": "fence",
    "shadows_cull_back_faces": "veils",
}
# rays outside the bound per mutation, of 2500 (the requirement is "at least one"; the figures are held too, so that this record stays true)
MUTATION_MISSES = {"cutout_commits": 336, "edge_on_every_shader": 343, "cutout_at_level_0": 7, "shadow_at_given_lod": 29, "shadow_uses_solid_alpha": 757, "o2_ignored": 44,
                   "stops_at_first_subtraction": 793, "closest_only": 793, "shadow_cutout_subtracts": 747, "shadows_cull_back_faces": 332}


@pytest.fixture(scope="module")
def solved(sample_data, oracle_lib):
    """name -> dict: one enumeration per culling mode, the oracle's own committing walks, and the two rules per case; shared by the tests below and left unchanged."""
    from oracle import oracle_py
    out = {}
    for name, data, seed, options, heights in AC.cases(sample_data):
        rays = AC.rays_of(data, seed, heights)
        o = oracle_py.OracleScene(data)
        try:
            o.render(W, H, images=False)
            cand = {c: R.candidates(o, rays, cull=bool(c)) for c in (0, 1)}
            bvh = {c: R.candidates(o, rays, cull=bool(c), brute_force=False) for c in (0, 1)}
            walks = {f: ray_rule.trace(o, rays, f) for f in (0, R.CULL_BACK_FACING, R.ACCEPT_FIRST_HIT)}
        finally:
            o.close()
        levels = M.texture_levels(data, MC.mipmapped(options))
        lods = AC.lods_of(seed, len(rays), options)
        out[name] = dict(data=data, levels=levels, rays=rays, lods=lods, cand=cand, bvh=bvh, walks=walks,
                         closest=R.closest_hit(data, levels, rays, cand[0], lods), closest_cull=R.closest_hit(data, levels, rays, cand[1], lods),
                         visibility=R.visibility(data, levels, rays, cand[0]))
    return out


def test_the_cases_keep_their_conditions(solved):
    assert list(solved) == AC.NAMES
    for name, s in solved.items():
        n = len(s["rays"])
        assert n == AC.RAYS + (AC.STEEP if name in AC.STACKED_TRANSLUCENT + AC.FENCES else 0)
        for key in ("closest", "closest_cull", "visibility"):
            assert s[key]["undecided"].mean() <= 0.02, (name, key)          # (an undecided ray is the only kind the device tests exclude)
        hits = (s["closest"]["hit"].view(np.int32)[:, 3] >= 0).sum()
        assert hits > n // 20, name
        two = int((s["visibility"]["subtracting"] >= 2).sum()); cut = int(s["closest"]["cutout_first"].sum())
        print("%-40s rays %4d candidates %5d hits %4d  two or more subtract %4d  closest candidate a cutout %4d  largest bound %.2e" %
              (name, n, len(s["cand"][0][0]), hits, two, cut, s["visibility"]["e"].max()))
        if name in AC.STACKED_TRANSLUCENT:
            assert two >= 100, name
            v = s["visibility"]["v"]
            assert ((v > 0.0) & (v < 1.0)).sum() >= 100 and ((v == 0.0) & ~s["visibility"]["by_o2"]).sum() >= 50, name          # sums on both sides of 1
        if name in AC.FENCES:
            assert cut >= 100, name
        assert s["visibility"]["e"].max() <= 1e-4, name          # the bound is not vacuous


def test_the_bvh_walk_enumerates_what_brute_force_does(solved):
    for name, s in solved.items():
        for c in (0, 1):
            (ia, ha), (ib, hb) = s["cand"][c], s["bvh"][c]
            assert np.array_equal(ia, ib) and np.array_equal(ha.view(np.uint32), hb.view(np.uint32)), (name, c)


def test_the_equivalences_hold_for_the_rule(solved):
    """K8: without a texture-edge shader the rule's closest hit is the committing walk's; on a scene whose instances are all O2-opaque visibility is 0 exactly where
    the accept-first walk hits and 1 where it misses."""
    for name in ("sample lds_cache=1", "sample lds_cache=0", "veils", "mixed"):
        s = solved[name]
        assert not R._edge(s["data"]).any()
        for key, flags in (("closest", 0), ("closest_cull", R.CULL_BACK_FACING)):
            assert not s[key]["undecided"].any()
            assert R.closest_matches(s[key], s["walks"][flags]).all(), (name, key)
    for name in ("sample lds_cache=1", "sample lds_cache=0", "texture edge at 0.3 exactly"):
        s = solved[name]
        assert R.shadow_opaque(s["data"], s["levels"]).all(), name
        hit = s["walks"][R.ACCEPT_FIRST_HIT].view(np.int32)[:, 3] >= 0
        v = s["visibility"]
        assert not v["undecided"].any() and np.array_equal(v["v"], np.where(hit, 0.0, 1.0)) and not v["e"].any(), name
        assert hit.sum() > 100 and (~hit).sum() > 100


def test_the_rule_names_the_instance_of_the_oracle_frame(sample_data, oracle_lib):
    """Camera rays of every pixel of the fence (one-level textures, depthBias 0: neither level nor key enters), back faces culled, the primary ray's window."""
    from oracle import oracle_py
    data = AC.fence(sample_data)
    px = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="xy"), axis=-1).reshape(-1, 2)
    rays = ray_rule.camera_rays(data, W, H, px)
    o = oracle_py.OracleScene(data)
    try:
        ref = o.render(W, H)
        cand = R.candidates(o, rays, cull=True)
    finally:
        o.close()
    hit = ref["primaryHit"]
    shown = np.where(hit[..., 3] == 0xFFFFFFFF, -1, (hit[..., 3] >> 24).astype(np.int64)).reshape(-1)
    rule = R.closest_hit(data, M.texture_levels(data), rays, cand)
    mine = rule["hit"].view(np.int32)[:, 3]
    decided = ~rule["undecided"]
    assert decided.mean() >= 0.98 and rule["cutout_first"].sum() >= 100 and len(set(mine[decided].tolist())) >= 4
    assert np.array_equal(mine[decided], shown[decided]), np.nonzero(decided & (mine != shown))[0][:8].tolist()


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_leaves_the_bound(solved, mutation):
    s = solved[MUTATION_CASES[mutation]]
    if mutation in R.CLOSEST_MUTATIONS:
        base = s["closest"]
        wrong = R.closest_hit(s["data"], s["levels"], s["rays"], s["cand"][0], s["lods"], mutate=mutation)
        out = ~R.closest_matches(base, wrong["hit"]) & ~wrong["undecided"]
    else:
        base = s["visibility"]
        wrong = R.visibility(s["data"], s["levels"], s["rays"], s["cand"][1 if mutation == "shadows_cull_back_faces" else 0], mutate=mutation, lods=s["lods"])
        out = ~base["undecided"] & ~wrong["undecided"] & (np.abs(base["v"] - wrong["v"]) > base["e"] + wrong["e"])
    print("%-28s on %-14s %4d of %4d rays outside the bound" % (mutation, MUTATION_CASES[mutation], int(out.sum()), len(out)))
    assert out.sum() >= 1
    assert int(out.sum()) == MUTATION_MISSES[mutation]
