"""CPU: the premises of tests/test_hip_shadow_fuzz.py, checked with the fp64 oracle alone for the very seeds and
builders the GPU tests use -- the structural cases occur, the oracle-compared scenes cast shadows and are decided
almost everywhere, the light-count ladder moves every high bit, the deterministic builders give the outcome they are
named for -- and the move of `_random_scene` left the primary fuzzes' random streams alone."""
import hashlib

import numpy as np
import pytest

import shadow_scenes as S
from oracle import np_oracle_tch

UNDECIDED_CAP = 0.005           # of hit (pixel, light) pairs, per oracle-compared scene set
SHADOWED_MIN = 0.01


def _digest(scene):
    h = hashlib.sha256()

    def walk(x):
        if isinstance(x, dict):
            for k in x:
                h.update(k.encode())
                walk(x[k])
        elif isinstance(x, np.ndarray):
            h.update(str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes())
        else:
            h.update(repr(x).encode())
    walk(scene)
    return h.hexdigest()


def test_random_scene_streams_did_not_move():
    """`_random_scene` moved from tests/test_hip_parity.py into tests/shadow_scenes.py: digests of the first scene of
    every stream the existing fuzzes draw (seeds 20240607, 77, 71, 41), recorded from the function before the move."""
    want = {20240607: "35ae2446ea85bd102f4499e3a0669b119186161f7dd1fe76a74a429cef5d755e",
            77: "3f0b2230a2ef8430b086c628fe10be64fe8078023070fc75aae5b28d6b282fb4",
            71: "f657c14accc472edf067318631e787e21ebe588c42163fea892a69dde79db222",
            41: "81eccf9fdb00e8a8c235a7a0c5175fc520c78f26e77a3c7eff10e5a80cd8c384"}
    for seed, digest in want.items():
        assert _digest(S._random_scene(np.random.RandomState(seed))) == digest, seed
    import test_hip_parity
    assert test_hip_parity._random_scene is S._random_scene


def test_every_structural_case_and_light_family_occurs():
    S.OCCURRED.clear()
    scenes = list(S.fuzz_scenes(S.FUZZ_SEED, S.FUZZ_COUNT))
    seen = dict(S.OCCURRED)
    for case in S.STRUCTURAL:
        assert seen.get(case, 0) >= 3, (case, seen)
    for family in S.LIGHT_FAMILIES:
        assert seen.get(family, 0) >= 10, (family, seen)
    assert seen["many_lights"] >= 3 and seen["view"] >= 50 and seen["no_view"] >= 50
    counts = {len(sc["lights"]["pos"]) for sc in scenes}
    assert counts >= {1, 2, 3, 4, 7} and len(counts & set(S.MANY_LIGHTS)) >= 3
    for sc in scenes:
        W, H = sc["camera"]["viewport"][2:]
        n_l = len(sc["lights"]["pos"])
        assert 33 <= W <= 200 and 17 <= H <= 160 and sc["camera"]["near"] >= 0.01 and 1 <= n_l <= 64
        assert n_l <= 7 or (S.primitive_count(sc) <= 700 and W <= 64 and H <= 48)
        for k in ("attenuation", "color_idx"):
            assert len(sc["lights"][k]) == n_l
    # the threshold family lands on both sides of the usable-view rule, the near-gap family on both sides of 0.1
    ratio = []
    for sc in scenes:
        b = S.scene_bounds(sc)
        if b["ok"]:
            d = np.linalg.norm(np.asarray(sc["lights"]["pos"], dtype=np.float64)[:, :3] - b["centre"], axis=1)
            ratio.extend(d / (1.3 * b["rad"] + 0.2))
    ratio = np.asarray(ratio)
    assert ((ratio > 0.95) & (ratio < 1.0)).sum() >= 5 and ((ratio > 1.0) & (ratio < 1.05)).sum() >= 5


def test_structural_scenes_are_what_they_are_named_for():
    """The cases `describe` cannot see in the scene alone, on a small frame with the oracle: the crowd's discs lie
    within a few tiles of a light's view, the far receivers lie far outside the bounding sphere."""
    rng = np.random.RandomState(3)
    crowd = S.random_shadow_scene(rng, "crowd")
    b = S.scene_bounds(crowd)
    view = S.light_views(crowd, b)[0]
    tile = 2.0 * view["half"] * view["dist"] / (view["res"] / S.TILE)          # a tile's width at the box centre
    d = crowd["objects"]["disk"]
    patch = np.abs(d["pos"][:, :3]).max(axis=1) <= 0.015
    assert patch.sum() >= 1000 and 0.03 * np.sqrt(3.0) / tile < 4.0                # the cube's diagonal, in tiles
    far = S.random_shadow_scene(rng, "far_receivers")
    far["camera"]["viewport"] = [0, 0, 33, 25]
    sc = S.oracle_input(far)
    res = np_oracle_tch.render(sc)
    hit = res["depth"] <= sc["camera"]["far"]
    b = S.scene_bounds(far)
    out = np.linalg.norm(res["pos"][hit] - b["centre"], axis=1) > 10.0 * b["rad"]
    assert out.mean() > 0.2
    assert all(v is not None for v in S.light_views(far, b)[:3])
    # one scene holds a fine and a coarse view: by k_light_frames' rule (tiles_fine falls as the view's extent
    # half * dist grows) the light at the threshold takes the fine view, the far one the coarse view
    mixed = S.random_shadow_scene(rng, "mixed_views")
    near, distant = S.light_views(mixed)[:2]
    assert near["dist"] < distant["dist"] and near["res"] == S.VIEW_RES_FINE and distant["res"] == S.VIEW_RES_COARSE
    assert near["tiles_fine"] < S.FINE_MAX_TILES < distant["tiles_fine"]


def test_oracle_compared_scenes_are_decided_and_cast_shadows():
    pairs = flips = dark = 0
    for scene in S.oracle_scenes(S.ORACLE_SEED, S.ORACLE_COUNT):
        for proj in ("perspective", "ortho"):
            scene["camera"]["proj_type"] = proj
            sc = S.oracle_input(scene)
            res = np_oracle_tch.render(sc, shadow=True)
            hit = res["depth"] <= sc["camera"]["far"]
            pairs += int(hit.sum()) * res["visibility"].shape[0]
            flips += int(S.undecided(sc, res).sum())
            dark += int((~res["visibility"][:, hit]).sum())
    print(f"oracle set: {pairs} hit pairs, undecided {flips / pairs:.4%}, shadowed {dark / pairs:.2%}")
    assert pairs > 50000
    assert flips / pairs <= UNDECIDED_CAP and dark / pairs >= SHADOWED_MIN


@pytest.fixture(scope="module")
def ladder():
    sc = S.oracle_input(S.ladder_scene())
    res = np_oracle_tch.render(sc, shadow=True)
    return sc, res, S.undecided(sc, res)


def test_ladder_scene_moves_every_high_bit(ladder):
    sc, res, und = ladder
    hit = res["depth"] <= sc["camera"]["far"]
    assert res["visibility"].shape[0] == 64 and 0.5 < hit.mean() < 1.0           # background pixels too
    for l in list(range(32, 64)) + [31]:
        bit = res["visibility"][l][hit & ~und[l]]
        assert bit.any() and not bit.all(), f"light {l} is {'visible' if bit.any() else 'blocked'} at every hit pixel"
    assert und[:, hit].mean() <= UNDECIDED_CAP and (~res["visibility"][:, hit]).mean() >= SHADOWED_MIN
    assert all(v is not None for v in S.light_views(S.ladder_scene()))          # 64 light views, 64 workspace slices


def test_deterministic_builders_give_their_named_outcome():
    pairs = flips = dark = 0
    for name, (scene, (light, outcome)) in S.deterministic_scenes().items():
        sc = S.oracle_input(scene)
        res = np_oracle_tch.render(sc, shadow=True)
        und = S.undecided(sc, res)
        hit = res["depth"] <= sc["camera"]["far"]
        r, c = S.centre_pixel(scene)
        assert hit[r, c] and not und[light, r, c], name
        assert res["visibility"][light, r, c] == (outcome == "lit"), f"{name}: expected {outcome}"
        pairs += int(hit.sum()) * und.shape[0]
        flips += int(und.sum())
        dark += int((~res["visibility"][:, hit]).sum())
    assert flips / pairs <= UNDECIDED_CAP and dark / pairs >= SHADOWED_MIN
    # the fragments of light_above_*: the centre pixel is within 0.1 of the light
    for receiver in ("disk", "plane"):
        scene = S.light_above_receiver(receiver)
        res = np_oracle_tch.render(S.oracle_input(scene))
        r, c = S.centre_pixel(scene)
        assert np.linalg.norm(res["pos"][r, c] - scene["lights"]["pos"][0, :3]) < 0.1
        assert (S.light_views(scene)[0] is not None) == (receiver == "plane")
    # the plane occluder leaves the light its view, the disc occluder does not
    for occluder in ("disk", "plane"):
        assert (S.light_views(S.occluder_behind_light(0.0999, occluder))[0] is not None) == (occluder == "plane")
    # coincident_tie: the fragment at the centre lies on disc 2; every pixel of the coincident spheres names sphere 3
    # (the lower index) and is lit although part of them face away from the light: the blocker is the pixel's own
    scene = S.coincident_tie()
    sc = S.oracle_input(scene)
    res = np_oracle_tch.render(sc, shadow=True)
    r, c = S.centre_pixel(scene)
    assert res["nearest"][r, c] == 2
    hit = res["depth"] <= sc["camera"]["far"]
    on_pair = hit & (res["nearest"] == 3)
    assert on_pair.sum() > 10 and not (hit & (res["nearest"] == 4)).any()
    assert res["visibility"][0][on_pair].all()
    away = np.sum(res["normal"] * (scene["lights"]["pos"][0, :3] - res["pos"]), axis=-1) < 0
    assert (on_pair & away).sum() > 3
