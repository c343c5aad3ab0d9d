"""hr_skin_pose_host (csrc/skin_math.h in a loop) against the numpy restatement (tests/skin_reference.py) on every case of tests/skin_cases.py,
compared as uint32 — no tolerance —, and hr_skin_bounds' box around every one of those outputs and around 200 random poses of the bar."""
import math

import numpy as np
import pytest

import skin_cases as sc
import skin_reference as sr

F = np.float32
CASES = sc.cases()


@pytest.fixture(scope="module")
def sk():
    from hybrid_rendering_amd import build as hb, skinning
    hb.build()
    return skinning


def test_the_case_table_covers_the_contracts_edges():
    by = {c["name"]: c for c in CASES}
    assert len(by) == len(CASES) >= 14
    assert by["bar_2_joints"]["arrays"]["verts"].shape == (64, 3, 3)
    w = by["slot_3_only"]["arrays"]["weights"].reshape(-1, 4)
    assert (w == F([0, 0, 0, 1])).all()
    w = by["slots_1_and_2"]["arrays"]["weights"].reshape(-1, 4)
    assert (w[:, 0] == 0).all() and (w[:, 1] != 0).any() and (w[:, 2] != 0).any()
    assert np.signbit(by["negative_zero_weight"]["arrays"]["weights"]).any()
    h = by["zero_weight_slot_names_a_non_finite_joint"]
    assert not np.isfinite(h["matrices"][3]).all() and (h["arrays"]["weights"][..., 2:] == 0).all() and (h["arrays"]["joints"][..., 2] == 3).all()
    assert {len(c["morph_weights"]) for c in CASES if c["morph_weights"] is not None} == {0, 1, 3}
    assert any(c["arrays"]["target_normals"] is None and c["arrays"]["target_positions"] is not None for c in CASES)
    assert any(c["morph_weights"] is not None and len(c["morph_weights"]) == 3 and (c["morph_weights"] == 0).sum() == 1 for c in CASES)
    assert np.abs(by["translations_of_1e6"]["matrices"][:, 12:15]).min() >= 1e6 - 100.0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pose_host_equals_the_reference_bit_for_bit(sk, case):
    a = case["arrays"]
    assert sk.check_desc(a) == 0
    rp, rn = sr.pose(a, case["matrices"], case["morph_weights"])
    hp, hn = sk.pose_host(a, case["matrices"], case["morph_weights"])
    sr.assert_same_bits(hp, rp, case["name"] + " positions")
    sr.assert_same_bits(hn, rn, case["name"] + " normals")
    if case.get("identity"):
        sr.assert_same_bits(hp, a["verts"], case["name"] + ": the identity keeps the rest position's bits")
    if case.get("hostile"):
        assert np.isfinite(hp).all() and np.isfinite(hn).all()
    if case.get("zero_normal"):
        zero = (hn.reshape(-1, 3) == 0).all(1)
        assert zero.any() and not zero.all(), "some normals go to exactly zero and are stored as they stand, the others are unit"
    moved = not case.get("identity")
    assert (sr.bits(hp) != sr.bits(a["verts"])).any() == moved


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_bounds_contain_every_case(sk, case):
    s = sk.Skin(None, case["arrays"])
    hp, _ = sk.pose_host(case["arrays"], case["matrices"], case["morph_weights"])
    sr.assert_box_contains(s.bounds(case["matrices"], case["morph_weights"]), hp, case["name"])
    s.close()


def test_bounds_contain_200_random_poses_of_the_bar(sk):
    """rotations, scales 0.5 to 2, translations up to 1e4, morph weights in [-1, 2] (one exactly 0 in every fourth pose, none given in every seventh)"""
    rng = np.random.RandomState(2024)
    a = sc.with_targets(sc.bar(3), 3, True, seed=9)
    s = sk.Skin(None, a)
    pivots = sc.bar_pivots(3)
    for i in range(200):
        pal = np.stack([sc.colmajor(sc.trs(rng.uniform(-1e4, 1e4, 3), rng.uniform(-1, 1, 3), rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 2.0, 3), pivots[j])) for j in range(3)])
        mw = rng.uniform(-1.0, 2.0, 3).astype(F)
        if i % 4 == 0:
            mw[i % 3] = 0.0
        hp, _ = sk.pose_host(a, pal, mw if i % 7 else None)
        box = s.bounds(pal, mw if i % 7 else None)
        sr.assert_box_contains(box, hp, f"pose {i}")
    s.close()


def test_random_skins_on_the_host(sk):
    """the generator the GPU sweep uses: host restatement against numpy on sizes around a wave and a block, 37 joints, 40 % empty slots"""
    for n_tris, n_joints, n_targets in ((1, 1, 0), (7, 2, 1), (22, 37, 3), (171, 37, 3)):
        a, pal, mw = sc.random_skin(n_tris, n_joints, n_targets, seed=n_tris)
        assert sk.check_desc(a) == 0
        rp, rn = sr.pose(a, pal, mw)
        hp, hn = sk.pose_host(a, pal, mw)
        sr.assert_same_bits(hp, rp, f"{n_tris} triangles positions")
        sr.assert_same_bits(hn, rn, f"{n_tris} triangles normals")
        s = sk.Skin(None, a)
        sr.assert_box_contains(s.bounds(pal, mw), hp, f"{n_tris} triangles")
        s.close()
