"""hr_deform_leaf_order without a GPU (csrc/deform_redeal.hip): the depth-first list of a tree's reference slots — slots of a node in slot
order (its internal children first: csrc/bvh.h), a leaf's triangles in offset order — relative to the tree's first reference.  It is the table the
device re-deal of a deformable mesh deals its sorted triangles by, so it is pinned here on hand-written node arrays against lists written out by
hand; and the C ABI of the re-deal is declared, exported and refuses NULL."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = {
    "hr_scene_rebuild_device": "hr_status hr_scene_rebuild_device(hr_scene* scene, void* stream);",
    "hr_scene_rebuild_meshes_device": "hr_status hr_scene_rebuild_meshes_device(hr_scene* scene, const uint32_t* mesh_idx, int32_t n, void* stream);",
    "hr_scene_device_rebuild_counts": "hr_status hr_scene_device_rebuild_counts(const hr_scene* scene, int64_t* rebuilds_enqueued, int64_t* launches_enqueued);",
    "hr_deform_leaf_order": "hr_status hr_deform_leaf_order(const void* nodes, int32_t n_nodes, uint32_t root, int32_t* slot_of_rank, int32_t capacity, int32_t* n);",
}


def node(n_internal, child_base, tri_base, leaves):
    """one 80-byte node (csrc/bvh.h): `n_internal` internal slots first, then `leaves` = [(count, offset), ...]; boxes left zero"""
    n = np.zeros(80, np.uint8)
    n[15] = n_internal | ((n_internal + len(leaves)) << 4)
    n[16:20] = np.array([child_base], np.uint32).view(np.uint8)
    n[20:24] = np.array([tri_base], np.uint32).view(np.uint8)
    for c in range(n_internal):
        n[24 + c] = 0x10
    for c, (count, offset) in enumerate(leaves):
        assert 1 <= count <= 4 and 0 <= offset < 32
        n[24 + n_internal + c] = (count << 5) | offset
    return n


def three_levels(node_base=0, tri_base=0):
    """root -> (node 1 -> node 3, node 2); the references lie breadth-first (root's leaf 0, node 1's 1-2, node 2's 3-5, node 3's 6-8)"""
    return np.stack([node(2, node_base + 1, tri_base + 0, [(1, 0)]),
                     node(1, node_base + 3, tri_base + 1, [(2, 0)]),
                     node(0, 0, tri_base + 3, [(1, 0), (2, 1)]),
                     node(0, 0, tri_base + 6, [(3, 0)])])


THREE_LEVELS_ORDER = [6, 7, 8, 1, 2, 3, 4, 5, 0]


def test_entry_points_are_declared_exported_and_refuse_null():
    from hybrid_rendering_amd import api
    hdr = re.sub(r"[ \t]+", " ", open(os.path.join(ROOT, "include", "hr_api_stages.h")).read())
    L = api.lib()
    for name, proto in PROTOTYPES.items():
        assert proto in hdr, name
        assert hasattr(L, name) and name in api.ABI_SYMBOLS and name in api.DEVICE_REDEAL_ARGTYPES, name
        getattr(L, name).argtypes = api.DEVICE_REDEAL_ARGTYPES[name]
    assert L.hr_api_revision() == 6
    a = C.c_int64(7)
    assert L.hr_scene_rebuild_device(None, None) == 1 and b"hr_scene_rebuild_device" in L.hr_last_error()
    assert L.hr_scene_rebuild_meshes_device(None, None, 0, None) == 1 and b"hr_scene_rebuild_meshes_device" in L.hr_last_error()
    assert L.hr_scene_device_rebuild_counts(None, C.byref(a), None) == 1 and b"hr_scene_device_rebuild_counts" in L.hr_last_error() and a.value == 7
    assert L.hr_deform_leaf_order(None, 1, 0, None, 0, None) == 1 and b"hr_deform_leaf_order" in L.hr_last_error()
    for cls, method in ((api.Scene, "rebuild_device"), (api.Scene, "device_rebuild_counts"), (api.InstancedScene, "rebuild_meshes_device")):
        assert callable(getattr(cls, method))


def test_one_node_with_leaves_of_every_count():
    """leaves of 3, 1, 4 and 2 triangles at offsets 1, 0, 6 and 4: slot order, then offset order"""
    from hybrid_rendering_amd import api
    nodes = np.stack([node(0, 0, 0, [(3, 1), (1, 0), (4, 6), (2, 4)])])
    assert api.deform_leaf_order(nodes).tolist() == [1, 2, 3, 0, 6, 7, 8, 9, 4, 5]
    assert api.deform_leaf_order(nodes, capacity=10).tolist() == [1, 2, 3, 0, 6, 7, 8, 9, 4, 5]


def test_depth_first_differs_from_the_breadth_first_reference_array():
    from hybrid_rendering_amd import api
    got = api.deform_leaf_order(three_levels()).tolist()
    assert got == THREE_LEVELS_ORDER and got != sorted(got)


def test_a_tree_inside_a_larger_array_with_a_tri_base_offset():
    """the same tree behind five other nodes, its references from 100 on: the list is relative to the tree's first reference"""
    from hybrid_rendering_amd import api
    front = np.stack([node(0, 0, 0, [(4, 0)])] * 5)
    nodes = np.concatenate([front, three_levels(node_base=5, tri_base=100)])
    assert api.deform_leaf_order(nodes, root=5).tolist() == THREE_LEVELS_ORDER
    assert api.deform_leaf_order(nodes, root=0).tolist() == [0, 1, 2, 3]
    assert api.deform_leaf_order(nodes, root=7).tolist() == [0, 1, 2]      # node 2 alone: references 103 .. 105


def test_errors_write_nothing():
    from hybrid_rendering_amd import api
    L = api.lib()
    L.hr_deform_leaf_order.argtypes = api.DEVICE_REDEAL_ARGTYPES["hr_deform_leaf_order"]
    nodes = np.ascontiguousarray(three_levels())
    out, n = np.full(16, -7, np.int32), C.c_int32(-7)

    def call(n_nodes, root, capacity):
        return L.hr_deform_leaf_order(C.c_void_p(nodes.ctypes.data), n_nodes, root, C.c_void_p(out.ctypes.data), capacity, C.byref(n))
    assert call(4, 0, 8) == 1 and b"hr_deform_leaf_order" in L.hr_last_error(), "capacity below the nine references"
    assert call(4, 4, 16) == 1, "a root outside the array"
    assert call(3, 0, 16) == 1, "node 1's child lies outside a three-node array"
    assert call(0, 0, 16) == 1 and call(4, 0, -1) == 1
    assert (out == -7).all() and n.value == -7
    assert call(4, 0, 9) == 0 and n.value == 9 and out[:9].tolist() == THREE_LEVELS_ORDER and (out[9:] == -7).all()
    with pytest.raises(api.HRError):
        api.deform_leaf_order(nodes, capacity=8)
    loop = nodes.copy()
    loop[3] = node(1, 0, 6, [(3, 0)])          # node 3 names the root as its child: not a tree
    assert L.hr_deform_leaf_order(C.c_void_p(loop.ctypes.data), 4, 0, C.c_void_p(out.ctypes.data), 16, C.byref(n)) == 1
