"""tests/bvh_check.check_packets and canonical_blas on a hand-made traversal copy (one instance, a single leaf of two triangles): what they
accept and what they notice, without a GPU. tests/test_refit.py repeats the exercise on a structure the device built."""
import numpy as np
import pytest

import bvh_check


def leaf_rule(n):
    return 2 if n <= 32 else 1


class Layout:
    InstanceOffset16, NodeOffset16, TriangleOffset16, LeafInstanceOffset16 = 0, 9, 14, 22
    InstanceCount, NodeCount, TriangleCount = 1, 1, 2


@pytest.fixture()
def blob():
    pos = np.random.default_rng(0).random((4, 3)).astype(np.float32)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    inst, node, tris = np.zeros(1, bvh_check.INST_DT), np.zeros(1, bvh_check.NODE_DT), np.zeros(2, bvh_check.TRI_DT)
    for p in range(2):
        tris[p]["v0"], tris[p]["v1"], tris[p]["v2"] = pos[idx[3 * p]], pos[idx[3 * p + 1]], pos[idx[3 * p + 2]]
        tris[p]["prim"] = p
    rows = np.zeros((2, 4), np.uint32); rows[:, :3] = idx.reshape(-1, 3)
    inst[0]["triCount"] = 2
    inst[0]["objectToWorld"] = inst[0]["worldToObject"] = np.eye(3, 4).reshape(-1)
    inst[0]["boxLo"], inst[0]["boxHi"] = pos.min(0), pos.max(0)
    buf = np.concatenate([a.view(np.uint8).reshape(-1) for a in (inst, node, tris, rows, inst)])
    return buf, [[(pos, idx)]]


def test_a_sound_copy_passes(blob):
    buf, geoms = blob
    bvh_check.check_blob(Layout, buf, leaf_rule)
    bvh_check.check_packets(Layout, buf, geoms)
    nodes, tris = bvh_check.canonical_blas(Layout, buf, 0, leaf_rule)
    assert len(nodes) == 0 and len(tris) == 2
    bvh_check.assert_records_equal(tris, tris.copy(), "packets")


def test_a_moved_vertex_a_repeated_primitive_and_stale_indices_are_noticed(blob):
    buf, geoms = blob
    d = buf.copy(); bvh_check.split(Layout, d)[2]["v1"][1, 2] += np.float32(1e-6)
    with pytest.raises(AssertionError, match="does not hold"):
        bvh_check.check_packets(Layout, d, geoms)
    d = buf.copy(); bvh_check.split(Layout, d)[2]["prim"][1] = 0
    with pytest.raises(AssertionError, match="more than once"):
        bvh_check.check_packets(Layout, d, geoms)
    d = buf.copy(); d[Layout.TriangleOffset16 * 16 + 2 * 48:].view("<u4")[1] = 3
    with pytest.raises(AssertionError, match="carries the vertex indices"):
        bvh_check.check_packets(Layout, d, geoms)
    with pytest.raises(AssertionError, match="1 geometry lists|packets for"):
        bvh_check.check_packets(Layout, buf, [[(geoms[0][0][0], geoms[0][0][1][:3])]])
    a, b = bvh_check.split(Layout, buf)[2], bvh_check.split(Layout, d)[2].copy()
    b["v0"][0, 0] = -b["v0"][0, 0]
    with pytest.raises(AssertionError, match="field v0 differs"):
        bvh_check.assert_records_equal(a, b, "packets")
