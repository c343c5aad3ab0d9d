"""The host side of the device re-build of a shared scene's top level (csrc/instance_math.h, csrc/instances_shared_rebuild.hip): the fixed 8-wide
shape hr_shared_top_fixed_shape gives an instance count, and the sort keys of hr_shared_top_sort_keys against a numpy restatement of the stated
arithmetic.  No GPU: both entry points are host code."""
import numpy as np
import pytest

from hybrid_rendering_amd import api, synth

SIZES = list(range(1, 601)) + [4095, 4096, 4097, 32768, 32769]


def levels_of(n):
    """node counts from the bottom level up: ceil(n / 8), ceil of that / 8, ... until one root stands"""
    out = [-(-n // 8)]
    while out[-1] > 1:
        out.append(-(-out[-1] // 8))
    return out


@pytest.fixture(scope="module")
def shapes():
    return {n: api.shared_top_fixed_shape(n) for n in SIZES}


def test_known_node_counts(shapes):
    for n, want in ((71, 12), (601, 89), (3301, 473), (7201, 1032)):
        nodes, _ = api.shared_top_fixed_shape(n)
        assert len(nodes) == want == sum(levels_of(n)), (n, len(nodes))


def test_the_shape_is_breadth_first_covers_every_leaf_once_and_is_as_shallow_as_possible(shapes):
    for n, (nodes, n_depths) in shapes.items():
        want_depths = 1
        while 8 ** want_depths < n:
            want_depths += 1
        assert n_depths == want_depths == len(levels_of(n)), (n, n_depths)                 # max(1, ceil(log8 n)) in integers
        assert len(nodes) == sum(levels_of(n)), (n, len(nodes))
        depth = nodes["depth"]
        assert depth[0] == 0 and np.all(np.diff(depth) >= 0) and np.all(np.diff(depth) <= 1) and depth[-1] == n_depths - 1, f"{n}: depths contiguous and in order"
        assert list(np.bincount(depth)) == levels_of(n)[::-1], n
        nc = nodes["n_internal"] + nodes["n_leaves"]
        if n == 1:
            assert len(nodes) == 1 and nc[0] == 1 and nodes["n_leaves"][0] == 1
        else:
            assert nc.min() >= 2 and nc.max() <= 8, (n, nc.min(), nc.max())
        assert np.all(nodes["axis"] == 0)
        # breadth-first: walking the slots in order, the internal children of slot s are the next unclaimed slots, one depth down
        next_child = 1
        for s, t in enumerate(nodes):
            assert (t["n_internal"] == 0) != (t["n_leaves"] == 0), f"{n}: slot {s} holds internal children or leaves, not both (internal before leaves)"
            if t["n_internal"]:
                assert t["child_base"] == next_child, f"{n}: slot {s}"
                assert np.all(depth[next_child:next_child + t["n_internal"]] == t["depth"] + 1)
                next_child += int(t["n_internal"])
        assert next_child == len(nodes), f"{n}: every internal slot is referenced exactly once"
        bottom = nodes[nodes["n_leaves"] > 0]
        assert np.all(bottom["depth"] == n_depths - 1), n
        assert bottom["leaf_base"][0] == 0 and np.array_equal(bottom["leaf_base"][1:], np.cumsum(bottom["n_leaves"])[:-1]) and bottom["n_leaves"].sum() == n, \
            f"{n}: leaves 0 .. n-1 exactly once and in order"
        lo, hi = n // len(bottom), -(-n // len(bottom))
        assert set(np.unique(bottom["n_leaves"])) <= {lo, hi}, f"{n}: dealt as evenly as possible"
        for d in range(n_depths - 1):                                                       # and so is every level above
            row = nodes[depth == d]["n_internal"]
            below = int((depth == d + 1).sum())
            assert row.sum() == below and set(np.unique(row)) <= {below // len(row), -(-below // len(row))}, (n, d)


def test_bad_arguments_are_status_codes():
    import ctypes as C
    L = api.lib()
    L.hr_shared_top_fixed_shape.argtypes = api.DEVICE_UPDATE_ARGTYPES["hr_shared_top_fixed_shape"]
    n, d = C.c_int32(0), C.c_int32(0)
    assert L.hr_shared_top_fixed_shape(0, None, 0, C.byref(n), C.byref(d)) == 1            # HR_ERR_INVALID_ARG
    buf = np.zeros(3, api.SHARED_TOP_NODE_DTYPE)
    assert L.hr_shared_top_fixed_shape(71, C.c_void_p(buf.ctypes.data), 3, C.byref(n), C.byref(d)) == 1 and n.value == 12, "capacity below the node count"
    assert not buf.view(np.int32).any(), "nothing written"


# ---- the sort key, restated ----------------------------------------------------------------------------------------------------------------------
def keys_np(boxes, bounds):
    """csrc/instance_math.h sort_key: per axis, in fp64, centre = (lo + hi) * 0.5; q = ((centre - bounds_lo) / (bounds_hi - bounds_lo)) * 1024;
    cell = floor(q) clamped to [0, 1023], 0 when q is not finite; x on bits 0, 3, ..., y on 1, 4, ..., z on 2, 5, ...; key = code << 32 | instance"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 6).astype(np.float64)
    bounds = np.asarray(bounds, np.float32).reshape(6).astype(np.float64)
    keys = np.zeros(len(boxes), np.uint64)
    with np.errstate(all="ignore"):
        for i, b in enumerate(boxes):
            code = 0
            for a in range(3):
                centre = (b[a] + b[3 + a]) * 0.5
                q = ((centre - bounds[a]) / (bounds[3 + a] - bounds[a])) * 1024.0
                cell = int(min(max(np.floor(q), 0.0), 1023.0)) if np.isfinite(q) else 0
                for bit in range(10):
                    code |= ((cell >> bit) & 1) << (3 * bit + a)
            keys[i] = (code << 32) | i
    return keys


def cornell_boxes(frame):
    from test_gpu_instances import _mats
    from test_gpu_instances_shared_device import instance_boxes_np
    isd = synth.instanced_cornell(600, seed=4)
    boxes = instance_boxes_np(isd, _mats(isd, 600, 4, frame))
    return boxes, np.concatenate([boxes[:, :3].min(0), boxes[:, 3:].max(0)])


@pytest.mark.parametrize("frame", [0, 90])
def test_keys_of_the_instanced_cornell_box(frame):
    boxes, bounds = cornell_boxes(frame)
    got, want = api.shared_top_sort_keys(boxes, bounds), keys_np(boxes, bounds)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
    codes = got >> np.uint64(32)
    assert len(np.unique(got)) == len(got) and codes.max() < 2 ** 30 and len(np.unique(codes)) > len(got) // 2, "30-bit codes that tell the instances apart"


def test_keys_of_crafted_boxes():
    inf = np.inf
    bounds = np.array([-1, -2, -3, 7, 6, 5], np.float32)
    boxes = np.array([
        [1, 1, 1, 2, 2, 2], [0, 0, 0, 3, 3, 3], [1.5, 1.5, 1.5, 1.5, 1.5, 1.5],   # all centres equal: told apart by the instance index alone
        [6, 5, 4, 8, 7, 6],                                                       # centre exactly on hi: cell 1024 clamps to 1023
        [-9, -9, -9, -8, -8, -8], [50, 50, 50, 60, 60, 60],                        # outside: clamped
        [-inf, 0, 0, inf, 1, 1], [0, 0, 0, inf, 1, 1], [-inf, -inf, -inf, 0, 0, 0], [np.nan, 0, 0, 1, 1, 1],   # infinite and NaN boxes: cell 0 on that axis
        [7, 6, 5, 7, 6, 5], [-1, -2, -3, -1, -2, -3],
    ], np.float32)
    got = api.shared_top_sort_keys(boxes, bounds)
    assert got.tobytes() == keys_np(boxes, bounds).tobytes()
    assert got[0] >> np.uint64(32) == got[1] >> np.uint64(32) == got[2] >> np.uint64(32) and list(got[:3] & np.uint64(0xffffffff)) == [0, 1, 2]
    assert got[3] >> np.uint64(32) == 2 ** 30 - 1 and got[5] >> np.uint64(32) == 2 ** 30 - 1 and got[4] >> np.uint64(32) == 0
    assert (int(got[6]) >> 32) & 0x09249249 == 0 and (int(got[7]) >> 32) & 0x09249249 == 0 and int(got[8]) >> 32 == 0, "an infinite box: cell 0"
    for flat in ([-1, -2, -3, -1, 6, 5], [-1, -2, -3, 7, -2, 5], [2, 2, 2, 2, 2, 2]):   # a zero extent on one axis / lo == hi: cell 0 there
        flat = np.array(flat, np.float32)
        got = api.shared_top_sort_keys(boxes, flat)
        assert got.tobytes() == keys_np(boxes, flat).tobytes(), flat
        zero_axes = [a for a in range(3) if flat[a] == flat[3 + a]]
        for a in zero_axes:
            assert not np.any((got >> np.uint64(32)) & np.uint64(0x09249249 << a)), f"axis {a} of {flat}"
    assert len(api.shared_top_sort_keys(np.zeros((0, 6), np.float32), bounds)) == 0
