"""tests/probe_vis_cases.py is not vacuous — from the numpy reference alone (tests/probe_vis_reference.py), no GPU, no library: every case draws a
real share of its pixels, names several probes, the depth cases really reject hits, the camera inside a sphere does not see that sphere, and a tie
between two probes goes to the smaller index."""
import numpy as np
import pytest

import probe_vis_cases as pc
import probe_vis_reference as ref

F = np.float32
DRAWING = [c.name for c in pc.CASES if not c.nothing]


def _n_probes(c):
    return int(np.prod(c.lattice[2]))


def _centres_on_screen(b):
    """indices of the probes whose centre projects inside the image, in front of the camera (float64)"""
    VP = np.asarray(b["ubo"]["view_proj"], np.float64).reshape(4, 4).T
    c = ref.probe_centres(b["grid"]).astype(np.float64)
    clip = np.concatenate([c, np.ones((len(c), 1))], 1) @ VP.T
    with np.errstate(all="ignore"):
        ndc = clip[:, :2] / clip[:, 3:4]
    return np.nonzero((clip[:, 3] > 0) & (np.abs(ndc) <= 1).all(1))[0].tolist()


@pytest.mark.parametrize("name", DRAWING)
def test_case_draws_a_real_share_and_names_several_probes(name):
    c, e = pc.BY_NAME[name], pc.expected(name)
    ids = e["probe_id"]
    drawn = float(np.mean(ids >= 0))
    assert ids.shape == (c.h, c.w) and e["color"].shape == (c.h, c.w, 4) and e["depth_out"].dtype == F
    if (c.w, c.h) == (1, 1):
        assert drawn == 1.0                      # a single pixel: drawn, and that is all it can say
        return
    assert 0.02 <= drawn <= 0.98, drawn
    if c.expect is not None:
        assert abs(drawn - c.expect) <= 0.01, (drawn, c.expect)      # the fraction the case was designed for, to the two digits it was stated in
    if c.hit_expect is not None:
        assert abs(float(np.mean(e["hit"] >= 0)) - c.hit_expect) <= 0.01
    # at least five distinct probes on a grid of more than four — or, where the camera cannot see that many, every probe whose centre is on screen
    # (thin_2x1x3: the two probes at z = 3 project to ndc y = 2.4 and 2.6; tiny_sphere: the camera looks out of the lattice's corner)
    b = pc.build(name)
    distinct = np.unique(ids[ids >= 0])
    on_screen = _centres_on_screen(b)
    assert len(distinct) >= min(5, _n_probes(c), len(on_screen)), (distinct, on_screen)
    if name in ("thin_2x1x3", "tiny_sphere"):
        assert len(on_screen) < 5 and set(on_screen) <= set(distinct.tolist())
    elif _n_probes(c) > 4:
        assert len(distinct) >= 5
    # a drawn texel carries its sphere's depth, in front of the G-buffer's; any other keeps depth_in
    assert (e["depth_out"][ids >= 0] < b["depth_in"][ids >= 0]).all()
    assert np.array_equal(e["depth_out"][ids < 0].view(np.uint32), b["depth_in"][ids < 0].view(np.uint32))
    assert np.array_equal(e["color"][ids < 0], b["color"][ids < 0]) and (e["color"][ids >= 0][:, 3] == 0x3c00).all()


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.depth[0] == "plane"])
def test_depth_cases_reject_hits(name):
    e = pc.expected(name)
    rejected = (e["hit"] >= 0) & (e["probe_id"] < 0)
    assert rejected.mean() >= 0.02, rejected.mean()
    assert (e["probe_id"][e["probe_id"] >= 0] == e["hit"][e["probe_id"] >= 0]).all()      # only the winner is tested: never a farther probe in its place


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.nothing])
def test_nothing_drawn_cases_draw_nothing(name):
    b, e = pc.build(name), pc.expected(name)
    assert (e["probe_id"] == -1).all() and np.array_equal(e["color"], b["color"]) and np.array_equal(e["depth_out"].view(np.uint32), b["depth_in"].view(np.uint32))
    if name == "nothing_depth_zero":
        assert (e["hit"] >= 0).mean() > 0.3      # the spheres are there; the depth test refuses every one
    else:
        assert (e["hit"] < 0).all()


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.avoid_probe])
def test_camera_inside_a_sphere_never_names_it(name):
    c, e = pc.BY_NAME[name], pc.expected(name)
    nx, ny, _ = c.lattice[2]
    p = c.avoid_probe[0] + c.avoid_probe[1] * nx + c.avoid_probe[2] * nx * ny
    centre = ref.probe_centres(pc.build(name)["grid"])[p]
    assert np.linalg.norm(centre - np.asarray(c.eye, F)) < 0.5          # the eye is inside it at both radii
    assert not (e["hit"] == p).any() and not (e["probe_id"] == p).any()
    assert (e["probe_id"] >= 0).mean() > 0.05


def test_hostile_atlases_reach_the_image():
    for name in ("hostile_atlas", "hostile_depth_atlas"):
        col = pc.expected(name)["color"].view(np.float16)[..., :3]
        assert np.isnan(col).sum() > 100 and np.isinf(col).sum() > 10, name


def test_path_pairs_straddle_half_a_step():
    for a, b in pc.PATH_PAIRS:
        ca, cb = pc.BY_NAME[a], pc.BY_NAME[b]
        half = F(0.5) * F(np.min(np.broadcast_to(np.asarray(ca.lattice[1], F), (3,))))
        assert F(ca.radius) == half and F(cb.radius) == np.nextafter(half, F(np.inf)) and ca.lattice == cb.lattice and ca.eye == cb.eye
        ia, ib = pc.expected(a)["probe_id"], pc.expected(b)["probe_id"]
        assert (ia == ib).mean() > 0.99          # the reference's ids agree nearly everywhere: the comparison of the two paths is not empty


def test_ties_resolve_to_the_smaller_index():
    """two probes mirrored about the ray: every operation of the test sees the same magnitudes, so both t are the same float"""
    grid = pc.lattice((-1.0, 0.0, 5.0), (2.0, 1.0, 1.0), (2, 1, 1))
    centres = ref.probe_centres(grid)
    assert centres.tolist() == [[-1.0, 0.0, 5.0], [1.0, 0.0, 5.0]]
    o, d = np.zeros(3, F), np.array([[0.0, 0.0, 1.0]], F)
    ok, t = ref.sphere_test(o, d[:, None, :], centres[None], 1.5)
    assert ok.all() and t[0, 0] == t[0, 1] and 3.0 < t[0, 0] < 5.0
    tb, p, n = ref.winners_of_rays(o, d, centres, 1.5)
    assert (int(p[0]), int(n[0])) == (0, 2) and tb[0] == t[0, 0]
    # ... whichever order the probes are listed in
    tb2, p2, _ = ref.winners_of_rays(o, d, centres[::-1], 1.5)
    assert int(p2[0]) == 0 and tb2[0] == tb[0]
    # and a nearer probe with a larger index still wins
    tb3, p3, _ = ref.winners_of_rays(o, d, np.array([[0.0, 0.0, 9.0], [0.0, 0.0, 5.0]], F), 1.0)
    assert int(p3[0]) == 1 and tb3[0] == F(4.0)
